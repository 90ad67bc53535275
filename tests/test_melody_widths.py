"""melody_size 12 and 16 (csrc/notes.hip: the five note-level kernels at W = 12 / 16) on the CPU interpreter: the oracle and
the HIP kernels against a fixture the reference produced at melody_size 16, every channel bucket of the applier's backward
that a small clip reaches, batched and bar-tiled plans, the forward-only stages with the plain mst_backward path, and the
one width rule that mst_widths_supported and mst_plan_create share."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import parity_cases as pc
from oracle import style_oracle as so
from tools.synth import synth_clip
from simutil import GOLDEN, flat_from_named, make_dims, rel, sim_native
from style import _native as nat
from test_tiled import run_tiled

SMALL = pc.SMALL
FIXTURE = 'small_melody16'
WIDTH_KEYS = ('beat', 'bar', 'nrf', 'style', 'melody', 'rhythm')


def load_fixture():
    z = np.load(os.path.join(GOLDEN, FIXTURE + '.npz'))
    widths = {k: int(v) for k, v in zip(WIDTH_KEYS, z['widths'])}
    assert widths == dict(SMALL, melody=16)
    return z, widths


def test_oracle_matches_the_reference_at_melody_16():
    """Same assertions and tolerances as test_oracle_golden.py::test_small_forward_loss_grads_adam (the fixture carries no
    post-Adam parameters: Adam does not depend on a width)."""
    TOL = 2e-5
    z, _ = load_fixture()
    flat = {k[3:]: torch.from_numpy(z[k]).clone().requires_grad_(True) for k in z.files if k.startswith('p0/')}
    Cn, R, T = (int(v) for v in z['crt'])
    unp, dens = bool(z['unpitched']), float(z['density'])
    assert unp
    mids = {}
    (info, xp, xu), losses = so.iteration(flat, synth_clip(0, Cn, R, T, unp, density=dens), mids=mids)
    for slot, key in (('pitched_beats', 'pitched_channels_encoder/0'), ('pitched_bars', 'pitched_channels_encoder/1'),
                      ('pitched_rhythm', 'pitched_rhythm_encoder/0'), ('style', 'style_encoder/0'), ('melody', 'melody_encoder/0'),
                      ('unpitched_beats', 'unpitched_channels_encoder/0'), ('unpitched_bars', 'unpitched_channels_encoder/1'),
                      ('unpitched_rhythm', 'unpitched_rhythm_encoder/0')):
        assert rel(mids[slot].detach(), z['mid/' + key]) < TOL, slot
    assert mids['melody'].shape[-1] == 16
    assert rel(xu.detach(), z['out/unpitched']) < TOL
    assert rel(info[0].detach(), z['out/instruments']) < TOL
    assert rel(info[1].detach(), z['out/mode']) < TOL
    assert rel(info[2].detach(), z['out/bpm']) < TOL
    assert rel(xp.detach(), z['out/pitched']) < TOL
    for k, v in losses.items():
        assert abs(v - float(z['loss0/' + k])) < 1e-5 * max(1, abs(v)), k
    assert set('loss0/' + k for k in losses) == set(k for k in z.files if k.startswith('loss0/'))
    for n, p in flat.items():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        ref = z['g0/' + n]
        if np.linalg.norm(ref) == 0:
            assert float(g.abs().max()) < 1e-7, n
            continue
        assert rel(g, ref) < 2e-4, n
    _, losses1 = so.iteration(flat, synth_clip(1, Cn, R, T, unp, density=dens))
    for k, v in losses1.items():
        assert abs(v - float(z['loss1/' + k])) < 1e-5 * max(1, abs(v)), k


def test_kernels_match_the_reference_at_melody_16():
    """parity_cases.golden_small at the fixture's widths: forward intermediates, the 15 loss leaves, every gradient, the
    second clip's total — on a NaN-poisoned arena."""
    native, device = sim_native(), 'cpu'
    z, widths = load_fixture()
    Cn, R, T = (int(v) for v in z['crt'])
    unp = bool(z['unpitched'])
    dims = make_dims(widths, Cn, R, T, unp)
    params, table = flat_from_named(native, dims, {k[3:]: z[k] for k in z.files if k.startswith('p0/')})
    plan = nat.Plan(native, dims, device)
    clip = synth_clip(0, Cn, R, T, unp, density=float(z['density']))
    pc.set_clip(plan, clip)
    gparams = torch.zeros_like(params)
    losses = torch.zeros(nat.N_LOSSES)
    xp, xu = pc.dev_clip(clip, device)
    pc.poison(plan)
    plan.train_iteration(params, gparams, xp, xu, losses)
    checks = [('pitched_beats', 'mid/pitched_channels_encoder/0'), ('pitched_bars', 'mid/pitched_channels_encoder/1'),
              ('pitched_rhythm', 'mid/pitched_rhythm_encoder/0'), ('style', 'mid/style_encoder/0'),
              ('melody', 'mid/melody_encoder/0'), ('instruments_pred', 'out/instruments'), ('mode_pred', 'out/mode'),
              ('bpm_pred', 'out/bpm'), ('pitched_pred', 'out/pitched'),
              ('unpitched_beats', 'mid/unpitched_channels_encoder/0'), ('unpitched_bars', 'mid/unpitched_channels_encoder/1'),
              ('unpitched_rhythm', 'mid/unpitched_rhythm_encoder/0'), ('unpitched_pred', 'out/unpitched')]
    for slot, key in checks:
        e = rel(plan.view(slot).numpy(), z[key])
        assert e < pc.TOL, (slot, e)
    n_leaves = 0
    for i, k in enumerate(nat.LOSS_KEYS):
        if 'loss0/' + k in z.files:
            n_leaves += 1
            assert abs(float(losses[i]) - float(z['loss0/' + k])) < 2e-5, (k, float(losses[i]), float(z['loss0/' + k]))
        else:
            assert np.isnan(float(losses[i])), k
    assert n_leaves == 15
    bad = []
    for pname, off, shape in table:
        ref = z['g0/' + pname].reshape(-1)
        got = gparams[off:off + ref.size].numpy()
        if np.linalg.norm(ref) < 1e-12:
            if np.abs(got).max() > 1e-6:
                bad.append((pname, 'nonzero', float(np.abs(got).max())))
        elif rel(got, ref) > 5e-4:
            bad.append((pname, rel(got, ref)))
    assert not bad, bad
    clip1 = synth_clip(1, Cn, R, T, unp, density=float(z['density']))
    pc.set_clip(plan, clip1)
    xp, xu = pc.dev_clip(clip1, device)
    plan.train_iteration(params, gparams, xp, xu, losses)
    assert abs(float(losses[0]) - float(z['loss1/total'])) < 2e-5


# psa_bwd2's channel buckets: C = 1, 2 one wave, C = 3 two waves, C = 5 four waves (three live)
@pytest.mark.parametrize('unp', [True, False])
@pytest.mark.parametrize('Cn', [1, 2, 3, 5])
@pytest.mark.parametrize('W', [12, 16])
def test_note_kernels_match_the_oracle(W, Cn, unp):
    R, T = (3, 2) if Cn <= 2 else (2, 1)
    pc.oracle_case(sim_native(), 'cpu', dict(SMALL, melody=W), Cn, R, T, unp, density=0.05, check_bitwise=True)


def test_batched_plan_equals_sequential_iterations():
    pc.batch_case(sim_native(), 'cpu', dict(SMALL, melody=16), 2, 2, 2, True, 3)


def test_batched_plan_on_the_mfma_gemm():
    pc.batch_case(sim_native(), 'cpu', dict(SMALL, melody=16), 2, 2, 1, True, 3, gemm_tile=64)


def test_bar_tiled_plan_equals_one_rank_plan():
    native = sim_native()
    w = dict(SMALL, melody=12)
    Cn, R, T, unp = 2, 4, 1, True
    dims = make_dims(w, Cn, R, T, unp)
    flat, _, _ = pc.random_params(native, dims, 3)
    clip = synth_clip(21, Cn, R, T, unp, density=0.05)
    plan = nat.Plan(native, dims, 'cpu')
    pc.set_clip(plan, clip)
    g1 = torch.zeros_like(flat)
    l1 = torch.zeros(nat.N_LOSSES)
    a, b = pc.dev_clip(clip, 'cpu')
    plan.train_iteration(flat.clone(), g1, a, b, l1)
    gt, lt, plans, _ = run_tiled(native, 'cpu', w, Cn, R, T, unp, [(0, 2), (2, 2)], clip, flat)
    for l in lt:
        assert torch.allclose(l, l1, atol=2e-6, equal_nan=True), (l, l1)
    assert rel(gt.numpy(), g1.numpy()) < 2e-5
    for k, (r0, rows) in enumerate([(0, 2), (2, 2)]):
        ref = plan.view('melody', (R, T * 10 * 56 * 12))[r0:r0 + rows]
        assert rel(plans[k].view('melody', (rows, T * 10 * 56 * 12)).numpy(), ref.numpy()) < 1e-5


def test_forward_only_stages_and_plain_backward():
    """The inference path: MST_STAGE_EXTRACT on clip A, then MST_STAGE_APPLY with clip B's style swapped in, against the
    oracle; then mst_backward of the apply stage from a seeded upstream gradient (psa_bwd2 with LOSS = false) against the
    oracle's autograd."""
    native = sim_native()
    w = dict(SMALL, melody=16)
    Cn, R, T = 2, 3, 2
    dims = make_dims(w, Cn, R, T, True)
    flat, named, table = pc.random_params(native, dims, 4)
    a, b = (synth_clip(k, Cn, R, T, True, density=0.05) for k in (40, 41))
    with torch.no_grad():
        style_a, melody_a, rhythm_a = so.extract_style(named, a['mode'], a['bpm'], a['pitched'], a['instruments_features'], a['unpitched'])
        style_b, _, _ = so.extract_style(named, b['mode'], b['bpm'], b['pitched'], b['instruments_features'], b['unpitched'])
    plan = nat.Plan(native, dims, 'cpu')
    pc.set_clip(plan, a)
    xp, xu = pc.dev_clip(a, 'cpu')
    pc.poison(plan)
    plan.forward(nat.STAGE_EXTRACT, flat, xp, xu)
    for k, ref in (('style', style_a), ('melody', melody_a), ('rhythm', rhythm_a)):
        assert rel(plan.view(k).numpy(), ref.numpy()) < pc.TOL, k
    # the swap: B's style on A's melody and rhythm, all of A's channels
    plan.view('style').copy_(style_b.reshape(-1))
    plan.forward(nat.STAGE_APPLY, flat, None, None)
    P = so.Params(named)
    leaves = [t.clone().requires_grad_(True) for t in (style_b, melody_a, rhythm_a)]
    xp_ref = so.pitched_style_applier(P.sub('pitched_style_applier'), leaves[0], leaves[1], leaves[2], a['instruments_features'])
    xu_ref = so.unpitched_style_applier(P.sub('unpitched_style_applier'), leaves[0], leaves[2])
    assert rel(plan.view('pitched_pred').numpy(), xp_ref.detach().numpy()) < pc.TOL
    assert rel(plan.view('unpitched_pred').numpy(), xu_ref.detach().numpy()) < pc.TOL
    # plain backward of the stage from a seeded gradient
    g = torch.Generator().manual_seed(9)
    g_xp, g_xu = torch.randn(xp_ref.shape, generator=g), torch.randn(xu_ref.shape, generator=g)
    ((xp_ref * g_xp).sum() + (xu_ref * g_xu).sum()).backward()
    plan.zero_grads(nat.STAGE_APPLY)
    for k in ('style', 'melody', 'rhythm'):
        plan.grad(k).zero_()
    plan.grad('pitched_pred').copy_(g_xp.reshape(-1))
    plan.grad('unpitched_pred').copy_(g_xu.reshape(-1))
    gparams = torch.zeros_like(flat)
    plan.backward(nat.STAGE_APPLY, flat, gparams, None, None)
    for k, leaf in zip(('style', 'melody', 'rhythm'), leaves):
        assert rel(plan.grad(k).numpy(), leaf.grad.numpy()) < pc.TOL, k
    seen = 0
    for pname, off, shape in table:
        gr = named[pname].grad
        n = int(np.prod(shape))
        if gr is None:
            assert float(gparams[off:off + n].abs().max()) == 0.0, pname
            continue
        seen += 1
        assert rel(gparams[off:off + n].numpy(), gr.reshape(-1).numpy()) < 5e-4, pname
    assert seen >= 10


@pytest.mark.parametrize('W,ok', [(4, True), (8, True), (12, True), (16, True),
                                  (2, False), (6, False), (10, False), (20, False), (32, False)])
def test_the_melody_width_rule(W, ok):
    native = sim_native()
    dims = make_dims(dict(SMALL, melody=W), 1, 2, 1, True)
    want = 0 if ok else -2                             # MST_OK / MST_ERR_UNSUPPORTED
    assert native.lib.mst_widths_supported(C.byref(dims)) == want
    st = C.c_int32(7)
    handle = native.lib.mst_plan_create(C.byref(dims), C.byref(st))
    assert st.value == want and bool(handle) == ok
    if handle:
        native.lib.mst_plan_destroy(handle)
