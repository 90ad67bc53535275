"""A dependency level's combine steps ride on its GEMM launch, and a train iteration's zero list on the first forward launch
(DESIGN.md 2).  Read through the C ABI on the CPU interpreter build: the launch lists say what is carried, and two train iterations
of the carrying plan are compared bit for bit with the same plan scheduled with no_merge = 1."""
import pytest

import combine_rider_cases as cr
import parity_cases as pc
from simutil import sim_native
from style import _native as nat


def test_bench_clip_combine_steps_and_zero_list_ride():
    native = sim_native()
    plan = nat.Plan(native, pc.make_dims(pc.FULL, 4, 16, 4, True), 'cpu')
    assert plan.gemm_tile == 32
    # 33 / 41 before: three forward and two backward combine first stages leave
    assert plan.launch_count(7, False) <= 30
    assert plan.launch_count(7, True) <= 39
    kinds = set()
    for backward in (False, True):
        rows, riders = cr.step_rows(plan, backward), plan.step_riders(7, backward)
        gemm_levels = {r[6] for r in rows if r[5] == cr.K_GEMM}
        for r, c in zip(rows, riders):
            if r[5] in (cr.K_COMB_F, cr.K_COMB_B):
                if r[6] in gemm_levels:
                    assert c == (2 if r[1] * r[2] > 4096 else 1), ('launched on its own beside a GEMM launch', r)
                else:
                    assert c == 0, ('alone on its level', r)
            if c:
                kinds.add(r[5])
        carried = plan.step_carried(7, backward)
        assert all(c == 0 or r[5] in (cr.K_GATHER, cr.K_SEGRED) for r, c in zip(rows, carried))
        assert sum(1 for r, c in zip(rows, carried) if c and r[5] == (cr.K_SEGRED if backward else cr.K_GATHER)) == 5
        assert sum(1 for c in carried if c) == 5
    assert kinds <= {cr.K_GATHER, cr.K_SEGRED, cr.K_COMB_F, cr.K_COMB_B} and cr.K_COMB_F in kinds and cr.K_COMB_B in kinds
    assert plan.zero_rides() == 1


# FULL 2,7,2: large sites of 4480 elements, nblk 5: 3.5 trips (a ragged last trip) and a ragged group of four;
# FULL 4,3,2: Cn = 4 fills the channel bound; SMALL: small widths; FULL 5,3,2: more than 4 channels, no combine rides, the zero
# list does; clips = 2: riders per clip
@pytest.mark.parametrize('widths,C,R,T,clips', [(pc.FULL, 2, 7, 2, 1), (pc.FULL, 4, 3, 2, 1), (pc.SMALL, 4, 3, 3, 1),
                                                (pc.FULL, 5, 3, 2, 1), (pc.SMALL, 2, 2, 2, 2)])
def test_carrying_plan_equals_the_unmerged_plan_bit_for_bit(widths, C, R, T, clips):
    cr.riders_equal_unmerged(sim_native(), 'cpu', widths, C, R, T, clips)


@pytest.mark.parametrize('opts', [dict(gemm_tile=64), dict(branches=1), dict(no_merge=1), dict(tile_r0=0, tile_rows=2)])
def test_other_plans_carry_nothing(opts):
    plan = nat.Plan(sim_native(), pc.make_dims(pc.FULL, 2, 4, 2, True), 'cpu', **opts)
    for mask in (7, 1, 2, 4):
        for backward in (False, True):
            assert not any(plan.step_riders(mask, backward))
    assert plan.zero_rides() == 0
