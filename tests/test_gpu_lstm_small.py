"""-m gpu: the one-wave LSTM kernels (H <= 16) on a real MI355X: bit for bit against the register-flavour kernels they replace
(the device build's contractions are part of that), against the oracle, and captured into a graph."""
import pytest
import torch

import combine_rider_cases as cr
import lstm_small_cases as ls
import parity_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def native():
    from style import _native as nat
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return nat.get()       # raises if libmst_amd.so is missing: no fallback


# the interpreter's cases, then FULL 4,16,4: the bench shape; FULL 1,40,1: S = 40 at H = 8 crosses the staging chunks of the
# one-wave kernels (30 steps forward, 17 backward) — at 16 steps the bench shape stays inside the first chunk; FULL 2,8,2 x 8
# clips: a batched plan on the 64x64 tiling whose H = 9 / H = 8 launches hold 64 / 8 sequences, too few for the grouped
# flavour (2048), so they take the one-wave kernels as the 64-clip bench regime's do
@pytest.mark.parametrize('widths,C,R,T,clips', [(pc.FULL, 2, 5, 2, 1), (pc.FULL, 1, 2, 1, 1), (pc.SMALL, 3, 2, 3, 1),
                                                (pc.SMALL, 2, 7, 2, 2), (pc.FULL, 4, 16, 4, 1), (pc.FULL, 1, 40, 1, 1),
                                                (pc.FULL, 2, 8, 2, 8)])
def test_one_wave_kernels_equal_the_register_flavour_bit_for_bit(native, widths, C, R, T, clips):
    a, b = ls.small_equals_register_flavour(native, DEV, widths, C, R, T, clips)
    assert a.plan.status() == 0 and b.plan.status() == 0


def test_reports_on_the_bench_shape(native):
    from style import _native as nat
    plan = nat.Plan(native, pc.make_dims(pc.FULL, 4, 16, 4, True), DEV)
    assert ls.expect_reports(plan) == 1
    for backward in (False, True):
        assert sorted(r[2] for _, r in ls.small_steps(plan, backward)) == [8, 9]


@pytest.mark.parametrize('widths,C,R,T', [(pc.FULL, 2, 5, 2), (pc.SMALL, 2, 3, 2)])
def test_oracle(native, widths, C, R, T):
    pc.oracle_case(native, DEV, widths, C, R, T, True, check_bitwise=True)


def test_graph_replay_equals_the_eager_iteration(native):
    eager = cr.Run(native, DEV, pc.FULL, 2, 7, 2)
    assert ls.small_steps(eager.plan, False) and ls.small_steps(eager.plan, True) and ls.expect_reports(eager.plan) == 1
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
