"""A dependency level's gathers and stage-1 segment reduces ride on its GEMM launch: one-stream, merged plans on
the 32x32 tiling carry them in gemm_kernel's grid instead of launching gather_kernel / segred_kernel beside it.  Read through the
C ABI on the CPU interpreter build: the launch lists say what is carried, and a train iteration of the carrying plan is compared
bit for bit with the same plan scheduled with no_merge = 1, which launches every member on its own kernel."""
import numpy as np
import pytest
import torch

import parity_cases as pc
from simutil import sim_native
from style import _native as nat
from tools.synth import synth_clip

K_GEMM, K_GATHER, K_SEGRED = 0, 1, 2
# workspace tensors with a name (include/mst_amd.h, mst_plan_tensor): activation and gradient of each are compared
NAMED = ['instr', 'mode', 'bpm', 'style', 'melody', 'rhythm', 'instruments_pred', 'mode_pred', 'bpm_pred', 'pitched_pred',
         'unpitched_pred', 'pitched_beats', 'pitched_bars', 'pitched_rhythm', 'unpitched_beats', 'unpitched_bars',
         'unpitched_rhythm']


def step_rows(plan, backward, mask=7):
    n = plan.lib.mst_plan_step_count(plan.handle, mask, int(backward))
    info = np.zeros((n, 8), np.int32)
    assert plan.lib.mst_plan_step_info(plan.handle, mask, int(backward), info.ctypes.data) == n
    return info.tolist()


def carried_steps(plan, backward, mask=7):
    """[(step_info row, carried code)] of the carried steps of a pass"""
    return [(r, c) for r, c in zip(step_rows(plan, backward, mask), plan.step_carried(mask, backward)) if c]


def test_bench_clip_gathers_and_segment_reduces_ride_on_their_levels_gemm_launch():
    native = sim_native()
    plan = nat.Plan(native, pc.make_dims(pc.FULL, 4, 16, 4, True), 'cpu')
    assert plan.gemm_tile == 32
    # 38 / 46 before: five gather launches and five segment-reduce stage-1 launches leave
    assert plan.launch_count(7, False) <= 33
    assert plan.launch_count(7, True) <= 41
    for backward, rider in ((False, K_GATHER), (True, K_SEGRED)):
        rows, carried = step_rows(plan, backward), plan.step_carried(7, backward)
        gemm_levels = {r[6] for r in rows if r[5] == K_GEMM}
        for r, c in zip(rows, carried):
            if r[5] in (K_GATHER, K_SEGRED):
                assert bool(c) == (r[6] in gemm_levels), ('launched on its own beside a GEMM launch', r)
            else:
                assert c == 0, ('only gathers and segment reduces are carried', r)
        assert sum(1 for r, c in zip(rows, carried) if c and r[5] == rider) == 5
    # per-stage lists (stages run separately): a rider is carried by a GEMM launch of its own stage, or not at all
    for mask in (1, 2, 4):
        for backward in (False, True):
            rows, carried = step_rows(plan, backward, mask), plan.step_carried(mask, backward)
            gemm_levels = {r[6] for r in rows if r[5] == K_GEMM}
            assert all(r[6] in gemm_levels for r, c in zip(rows, carried) if c)


def run_iteration(native, widths, C, R, T, **opts):
    dims = pc.make_dims(widths, C, R, T, True)
    flat, _, _ = pc.random_params(native, dims)
    clip = synth_clip(5, C, R, T, True, density=0.05)
    plan = nat.Plan(native, dims, 'cpu', **opts)
    pc.set_clip(plan, clip)
    g = torch.zeros_like(flat)
    losses = torch.zeros(nat.N_LOSSES)
    xp, xu = pc.dev_clip(clip, 'cpu')
    plan.train_iteration(flat, g, xp, xu, losses)
    return plan, g, losses


def bits(t):
    return t.contiguous().view(torch.int32)       # bit patterns: equal NaNs compare equal too


# SMALL 4,3,3: the conv-gradient segment reduce sums 180 rows, so it is two-stage (chunks of 64) and its first stage rides;
# every shape has the rhythm encoders' broadcast-sum gather (linear_bcast) on a level with GEMMs
@pytest.mark.parametrize('widths,C,R,T,two_stage', [(pc.SMALL, 3, 2, 3, False), (pc.SMALL, 4, 3, 3, True), (pc.FULL, 2, 3, 2, False)])
def test_carrying_plan_equals_the_unmerged_plan_bit_for_bit(widths, C, R, T, two_stage):
    native = sim_native()
    plan, g, losses = run_iteration(native, widths, C, R, T)
    ref, g_ref, losses_ref = run_iteration(native, widths, C, R, T, no_merge=1)
    # the plan under test really carries riders ...
    fwd, bwd = carried_steps(plan, False), carried_steps(plan, True)
    assert fwd and all(r[5] == K_GATHER and c == 1 for r, c in fwd)
    assert bwd and all(r[5] == K_SEGRED for r, c in bwd)
    # ... among them the sum gather of both rhythm encoders (two members of `rhythm` columns; pitched: rows = C x R x T, five
    # broadcast blocks) ...
    assert [r for r, c in fwd if r[:3] == [C * R * T, widths['rhythm'], 5] and r[4] == 2]
    # ... and, where the shape has one, a two-stage segment reduce whose second stage stays a launch
    assert any(c == 2 for r, c in bwd) == two_stage
    # the unmerged plan carries nothing
    assert not carried_steps(ref, False) and not carried_steps(ref, True)
    assert ref.launch_count(7, True) > 3 * plan.launch_count(7, True)
    assert torch.equal(bits(g), bits(g_ref))
    assert torch.equal(bits(losses), bits(losses_ref))
    for name in NAMED:
        assert torch.equal(bits(plan.view(name)), bits(ref.view(name))), name
        assert torch.equal(bits(plan.grad(name)), bits(ref.grad(name))), ('gradient of', name)
    # both plans lay the workspace out alike: every activation, gradient and scratch element
    assert plan.ws.numel() == ref.ws.numel()
    assert torch.equal(bits(plan.ws), bits(ref.ws))


def test_batched_plan_on_the_small_tiling_carries_per_clip():
    # up to five clips per launch stay on the 32x32 tiling: the grid is clip-major, a clip's block range holds its riders and its
    # GEMM members (results: tests/test_sim_parity.py, batched equals sequential)
    native = sim_native()
    dims = pc.make_dims(pc.SMALL, 2, 2, 2, True, clips=3)
    plan = nat.Plan(native, dims, 'cpu')
    one = nat.Plan(native, pc.make_dims(pc.SMALL, 2, 2, 2, True), 'cpu')
    assert plan.gemm_tile == 32
    for backward in (False, True):
        got = [(r[5], r[6], r[4], c) for r, c in carried_steps(plan, backward)]
        assert got and got == [(k, lv, 3 * n, c) for (k, lv, n, c) in [(r[5], r[6], r[4], c) for r, c in carried_steps(one, backward)]]


@pytest.mark.parametrize('opts', [dict(gemm_tile=64), dict(branches=1), dict(no_merge=1), dict(tile_r0=0, tile_rows=2)])
def test_other_plans_carry_nothing(opts):
    native = sim_native()
    plan = nat.Plan(native, pc.make_dims(pc.FULL, 2, 4, 2, True), 'cpu', **opts)
    for mask in (7, 1, 2, 4):
        for backward in (False, True):
            assert not any(plan.step_carried(mask, backward))
            # every step is a launch (two for a two-stage segment reduce or combine), plus the slab reduces of a backward pass
            rows = step_rows(plan, backward, mask)
            assert plan.launch_count(mask, backward) >= len(rows) + (bin(mask).count('1') if backward else 0)


def test_plan_that_chooses_the_large_tiling_carries_nothing():
    native = sim_native()
    plan = nat.Plan(native, pc.make_dims(pc.SMALL, 2, 2, 2, True, clips=8), 'cpu')
    assert plan.gemm_tile == 64
    assert not any(plan.step_carried(7, False)) and not any(plan.step_carried(7, True))
