"""Shared by test_combine_riders.py (CPU interpreter) and test_gpu_combine_riders.py: a plan whose GEMM launches carry their level's
combine steps and whose first forward launch clears the zero list, against the same plan scheduled with no_merge = 1 (every
member on its own kernel), bit for bit over two train iterations on a NaN-poisoned workspace."""
import numpy as np
import torch

import parity_cases as pc
from style import _native as nat
from tools.synth import synth_clip

K_GEMM, K_GATHER, K_SEGRED, K_COMB_F, K_COMB_B = 0, 1, 2, 5, 6
# workspace tensors with a name (include/mst_amd.h, mst_plan_tensor): activation and gradient of each are compared
NAMED = ['instr', 'mode', 'bpm', 'style', 'melody', 'rhythm', 'instruments_pred', 'mode_pred', 'bpm_pred', 'pitched_pred',
         'unpitched_pred', 'pitched_beats', 'pitched_bars', 'pitched_rhythm', 'unpitched_beats', 'unpitched_bars',
         'unpitched_rhythm']


def step_rows(plan, backward, mask=7):
    n = plan.lib.mst_plan_step_count(plan.handle, mask, int(backward))
    info = np.zeros((n, 8), np.int32)
    assert plan.lib.mst_plan_step_info(plan.handle, mask, int(backward), info.ctypes.data) == n
    return info.tolist()


def bits(t):
    return t.contiguous().view(torch.int32)       # bit patterns: equal NaNs compare equal too


class Run:
    """One plan with its inputs; iterate() poisons on request and runs one train iteration."""

    def __init__(self, native, device, widths, C, R, T, clips=1, **opts):
        self.device = device
        dims = pc.make_dims(widths, C, R, T, True, clips=clips)
        flat, _, _ = pc.random_params(native, pc.make_dims(widths, C, R, T, True))
        self.params = flat.to(device)
        self.plan = nat.Plan(native, dims, device, **opts)
        cl = [synth_clip(5 + k, C, R, T, True, density=0.05) for k in range(clips)]
        for k, c in enumerate(cl):
            self.plan.set_inputs(mode=c['mode'], bpm=c['bpm'], instr=c['instruments_features'], used=c['used_instruments'],
                                 bpm_target=float(c['bpm_int']), clip=k)
        self.xp = torch.cat([c['pitched'] for c in cl]).contiguous().to(device)
        self.xu = torch.cat([c['unpitched'] for c in cl]).contiguous().to(device)
        self.g = torch.zeros_like(self.params)
        self.losses = torch.zeros(clips, nat.N_LOSSES, device=device) if clips > 1 else torch.zeros(nat.N_LOSSES, device=device)
        self.clips = clips

    def iterate(self, poison):
        if poison:
            pc.poison(self.plan)
        self.plan.train_iteration(self.params, self.g, self.xp, self.xu, self.losses)


def assert_same(a, b):
    assert torch.equal(bits(a.g), bits(b.g))
    assert torch.equal(bits(a.losses), bits(b.losses))
    for k in range(a.clips):
        kw = dict(clip=k) if a.clips > 1 else {}
        for name in NAMED:
            assert torch.equal(bits(a.plan.view(name, **kw)), bits(b.plan.view(name, **kw))), (name, k)
            assert torch.equal(bits(a.plan.grad(name, **kw)), bits(b.plan.grad(name, **kw))), ('gradient of', name, k)
    # both plans lay the workspace out alike: every activation, gradient and scratch element
    assert a.plan.ws.numel() == b.plan.ws.numel()
    assert torch.equal(bits(a.plan.ws), bits(b.plan.ws))


def expect_riders(plan, C):
    """what the carrying plan must carry: with C <= 4 every combine step that shares a level with a GEMM launch (1 small, 2 large),
    with more channels no combine step; the zero list either way"""
    seen = 0
    for backward in (False, True):
        rows, riders = step_rows(plan, backward), plan.step_riders(7, backward)
        gemm_levels = {r[6] for r in rows if r[5] == K_GEMM}
        for r, c in zip(rows, riders):
            if r[5] in (K_COMB_F, K_COMB_B):
                large = r[1] * r[2] > 4096
                want = 0 if (C > 4 or r[6] not in gemm_levels) else (2 if large else 1)
                assert c == want, (r, c, want)
                seen += c != 0
            else:
                assert c == 0 or r[5] in (K_GATHER, K_SEGRED), r
    assert (seen > 0) == (C <= 4)
    assert plan.zero_rides() == 1


def riders_equal_unmerged(native, device, widths, C, R, T, clips=1):
    a = Run(native, device, widths, C, R, T, clips)
    b = Run(native, device, widths, C, R, T, clips, no_merge=1)
    expect_riders(a.plan, C)
    assert not any(b.plan.step_riders(7, False)) and not any(b.plan.step_riders(7, True)) and b.plan.zero_rides() == 0
    for it in range(2):          # the first on a poisoned workspace, the second on what the first left
        a.iterate(poison=it == 0)
        b.iterate(poison=it == 0)
        assert_same(a, b)
    return a, b
