"""-m gpu: the combine steps and the zero list inside gemm_kernel launches on a real MI355X, bit for bit against the plan that
launches every member on its own kernel; against the oracle; and captured into a graph."""
import pytest
import torch

import combine_rider_cases as cr
import parity_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def native():
    from style import _native as nat
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return nat.get()       # raises if libmst_amd.so is missing: no fallback


@pytest.mark.parametrize('C,R,T,clips', [(2, 7, 2, 1), (4, 3, 2, 1), (5, 3, 2, 1), (2, 7, 2, 2)])
def test_carrying_plan_equals_the_unmerged_plan_bit_for_bit(native, C, R, T, clips):
    a, b = cr.riders_equal_unmerged(native, DEV, pc.FULL, C, R, T, clips)
    assert a.plan.status() == 0 and b.plan.status() == 0


def test_oracle_with_ragged_large_sites(native):
    pc.oracle_case(native, DEV, pc.FULL, 2, 7, 2, True, check_bitwise=True)


def test_graph_replay_equals_the_eager_iteration(native):
    eager = cr.Run(native, DEV, pc.FULL, 2, 7, 2)
    cr.expect_riders(eager.plan, 2)
    eager.iterate(poison=True)
    torch.cuda.synchronize()
    run = cr.Run(native, DEV, pc.FULL, 2, 7, 2)
    pc.poison(run.plan)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run.iterate(poison=False)          # warm: graph capture must not be the first use
        run.g.zero_()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run.iterate(poison=False)
    for rep in range(3):
        run.g.zero_()
        pc.poison(run.plan)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cr.bits(run.g), cr.bits(eager.g)), rep
        assert torch.equal(cr.bits(run.losses), cr.bits(eager.losses)), rep
        assert run.plan.status() == 0
