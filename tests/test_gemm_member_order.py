"""Member order inside a GEMM launch (plan.hip, schedule_pass), read through mst_plan_step_gemms on the CPU interpreter build:
one-clip plans (32x32 tiling) dispatch the member with the longest dependent k chain first; plans on the 64x64 tiling keep the
order in which the model emitted the members; the number of launches does not depend on it."""
import pytest

import parity_cases as pc
from simutil import sim_native
from style import _native as nat

K_GEMM, K_GEMM_FOLD = 0, 25


def launches(plan, backward):
    """[(members, kinds)] of every GEMM launch step of the whole-model pass"""
    out = []
    for st in range(plan.lib.mst_plan_step_count(plan.handle, 7, int(backward))):
        members = plan.step_gemms(7, backward, st)
        if members:
            kinds = plan.step_gemm_kinds(7, backward, st)
            assert len(kinds) == len(members)
            out.append((members, kinds))
    return out


def k_tiles(member, kd):
    M, N, K, splits, fold_rows, wgs = member
    kr = -(-K // splits)
    assert kd == (32 if kr <= 32 else (64 if kr <= 64 else 128))         # the kernel's rule for the k-tile depth
    return -(-kr // kd)


def is_subsequence(part, whole):
    it = iter(whole)
    return all(any(x == y for y in it) for x in part)


@pytest.mark.parametrize('C,R,T', [(4, 16, 4), (2, 7, 2)])           # the bench shape; the rider tests' shape
def test_one_clip_launches_list_the_longest_member_first(C, R, T):
    native = sim_native()
    dims = pc.make_dims(pc.FULL, C, R, T, True)
    plan = nat.Plan(native, dims, 'cpu')
    assert plan.gemm_tile == 32
    emitted = nat.Plan(native, dims, 'cpu', no_merge=1)
    reordered = 0
    for backward in (False, True):
        order = [m for members, _ in launches(emitted, backward) for m in members]
        for members, kinds in launches(plan, backward):
            tiles = [k_tiles(m, kd) for m, (_, kd) in zip(members, kinds)]
            assert tiles == sorted(tiles, reverse=True), (backward, members, tiles)
            reordered += not is_subsequence(members, order)
    assert reordered > 0, 'no launch of this shape has a longer member behind a shorter one: the test shows nothing'


def test_bench_shape_launch_count_is_unchanged():
    plan = nat.Plan(sim_native(), pc.make_dims(pc.FULL, 4, 16, 4, True), 'cpu')
    assert plan.lib.mst_plan_launch_count(plan.handle, 7, 0) == 30
    assert plan.lib.mst_plan_launch_count(plan.handle, 7, 1) == 38


@pytest.mark.parametrize('C,R,T', [(4, 16, 4), (2, 7, 2)])
def test_plans_on_the_64x64_tiling_keep_the_emitted_order(C, R, T):
    native = sim_native()
    dims = pc.make_dims(pc.FULL, C, R, T, True)
    plan = nat.Plan(native, dims, 'cpu', gemm_tile=64)
    emitted = nat.Plan(native, dims, 'cpu', gemm_tile=64, no_merge=1)
    assert plan.gemm_tile == 64 and emitted.gemm_tile == 64
    merged = 0
    for backward in (False, True):
        order = [m for members, _ in launches(emitted, backward) for m in members]
        assert sorted(order) == sorted(m for members, _ in launches(plan, backward) for m in members)
        for members, kinds in launches(plan, backward):
            assert is_subsequence(members, order), (backward, members)
            assert all(kd == 32 for _, kd in kinds)
            merged += len(members) > 1
    assert merged > 0
