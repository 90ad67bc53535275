"""Shared cases and yardsticks of the held-out evaluation path (mst_roll_metrics, mst_eval_iteration), used by the
CPU-interpreter tests and the GPU tests alike: everything here works on torch tensors of any device and a binding of the C ABI.

The feature has no reference counterpart, so the yardstick is a float64 numpy restatement of the record table of
include/mst_amd.h, written here.  The hard accidentals are those of oracle.style_oracle.hard_output.  Counts must be equal;
the two sums of non-negative fp32 terms must agree within group_cells * 2^-52 relative (each summation order is within
n * 2^-53 of the exact sum)."""
import numpy as np
import torch

import parity_cases as pc
from oracle import style_oracle as so
from simutil import make_dims
from style import _native as nat
from tools.synth import synth_clip

W = 8                   # MST_METRIC_WORDS
S = 1024                # cells of a group one workgroup owns (ROLL_SLICE, csrc/loss_optim.hip)
NAN = float('nan')
ERR_ARG, ERR_UNSUPPORTED = -1, -2
SIZES = [(1, 1), (1, 1023), (1, 1024), (1, 1025), (3, 1025), (2, 2 * 1024 + 777)]
MANY_PARTIALS = (1, 257 * 1024 + 3)         # more partials than the finishing workgroup has lanes


def bits(t):
    t = torch.as_tensor(t).detach().cpu().contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def same_bits(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- the yardstick
def yardstick(pred, target, n_groups, group_cells, nfeat):
    """(n_groups, 8) float64 records of two host rolls, straight from the table."""
    p = torch.as_tensor(pred).detach().cpu().reshape(n_groups, group_cells, nfeat)
    t = torch.as_tensor(target).detach().cpu().reshape(n_groups, group_cells, nfeat).numpy()
    hard = so.hard_output(p.clone()).numpy()          # (it zeroes velocities of its input: a clone)
    p = p.numpy()
    f32 = np.float32
    with np.errstate(invalid='ignore'):
        on = p[..., 1] > f32(.01)                     # a NaN velocity is off
        want = t[..., 1] > f32(0.)
        tp = on & want
        out = np.zeros((n_groups, W), dtype=np.float64)
        out[:, 0] = group_cells
        out[:, 1], out[:, 2], out[:, 3] = on.sum(1), want.sum(1), tp.sum(1)
        if nfeat == 5:
            out[:, 4] = (tp & (hard[..., 2:] == t[..., 2:]).all(-1)).sum(1)
        vel = np.abs(p[..., 1] - t[..., 1]).astype(f32).astype(np.float64)
        dur = np.abs(p[..., 0] - np.fmin(t[..., 0], f32(6.))).astype(f32).astype(np.float64)
        out[:, 5] = np.where(tp, vel, 0.).sum(1)
        out[:, 6] = np.where(tp, dur, 0.).sum(1)
    return out


def song_info_yardstick(instr_logits, instr_target, mode_logits, mode_target, bpm_pred, bpm_target):
    f = lambda x: torch.as_tensor(x).detach().cpu().reshape(-1).numpy().astype(np.float32)
    il, it, ml, mt, bp, bt = (f(x) for x in (instr_logits, instr_target, mode_logits, mode_target, bpm_pred, bpm_target))
    on, want = il > 0, it > .5
    return np.array([len(il), on.sum(), want.sum(), (on & want).sum(), float(np.argmax(ml) == np.argmax(mt)),
                     float(np.abs(np.float32(bp[0] - bt[0]))), 0., 0.], dtype=np.float64)


def check_records(got, want, group_cells):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, W), np.asarray(want, dtype=np.float64).reshape(-1, W)
    assert got.shape == want.shape, (got.shape, want.shape)
    for k in (0, 1, 2, 3, 4, 7):
        assert np.array_equal(got[:, k], want[:, k]), (k, got[:, k], want[:, k])
    for k in (5, 6):
        for g, w in zip(got[:, k], want[:, k]):
            if np.isnan(w):
                assert np.isnan(g), (k, g, w)
            else:
                assert abs(g - w) <= group_cells * 2. ** -52 * w, (k, g, w, abs(g - w))


def counts_not_trivial(records):
    """0 < TP < n_pred and TP < n_tgt over the sum of the records."""
    r = np.asarray(records, dtype=np.float64).reshape(-1, W).sum(0)
    return 0 < r[3] < r[1] and r[3] < r[2]


# ---- rolls
def random_pair(n_cells, nfeat, seed):
    """A target roll at 30 % density and a prediction of it: most notes kept with jittered velocity and duration, a fifth
    missed, a third of the kept ones scaled to around the .01 threshold, false positives in 5 % of the silent cells, soft
    accidentals, some target durations beyond the clamp at 6."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, generator=g)
    live = r(n_cells) < .3
    if n_cells == 1:
        live[:] = True
    target = torch.zeros(n_cells, nfeat)
    target[:, 0] = r(n_cells) * 8. * live
    target[:, 1] = (.1 + .9 * r(n_cells)) * live
    pred = torch.zeros(n_cells, nfeat)
    pred[:, 0] = (target[:, 0].clamp(max=6.) + r(n_cells) - .5).abs() * live
    kept = live & (r(n_cells) > .2)
    pred[:, 1] = (target[:, 1] + .2 * (r(n_cells) - .5)).clamp(min=.02) * kept
    quiet = r(n_cells) < .3
    pred[:, 1] = torch.where(quiet, pred[:, 1] * .02, pred[:, 1])
    extra = ~live & (r(n_cells) < .05)
    pred[:, 1] = torch.where(extra, r(n_cells), pred[:, 1])
    pred[:, 0] = torch.where(extra, 3. * r(n_cells), pred[:, 0])
    if nfeat == 5:
        which = torch.randint(0, 3, (n_cells,), generator=g)
        for a in range(3):
            target[:, 2 + a] = (which == a).float() * live
        pred[:, 2:] = (.6 * target[:, 2:] + .5 * r(n_cells, 3)) * (pred[:, 1:2] != 0)
    return pred.contiguous(), target.contiguous()


def near_threshold(x, seed):
    """A third of the velocities scaled to around the .01 threshold (as the sparse-output tests do it)."""
    g = torch.Generator().manual_seed(seed)
    x = x.clone()
    quiet = torch.rand(x.shape[:-1], generator=g) < .3
    x[..., 1] = torch.where(quiet, x[..., 1] * .02, x[..., 1])
    return x


def synth_pair(key, seed=3, crt=(3, 2, 3)):
    """A synthetic clip's roll as the target and a prediction like a model's: the target's notes with a third of the
    velocities around the threshold, 1 % false positives, jittered durations, soft accidentals."""
    clip = synth_clip(seed, *crt, True, density=.05)
    target = clip[key].contiguous()
    g = torch.Generator().manual_seed(seed + 100)
    r = lambda *shape: torch.rand(*shape, generator=g)
    pred = near_threshold(target, seed + 1)
    extra = (target[..., 1] == 0) & (r(target.shape[:-1]) < .01)
    pred[..., 1] = torch.where(extra, r(target.shape[:-1]), pred[..., 1])
    pred[..., 0] = (pred[..., 0] + .3 * (r(target.shape[:-1]) - .5)).abs() * (pred[..., 1] != 0)
    if target.shape[-1] == 5:
        pred[..., 2:] = (.6 * target[..., 2:] + .5 * r(target.shape[:-1] + (3,))) * (pred[..., 1:2] != 0)
    n_groups = target.shape[1]
    return pred.contiguous(), target, n_groups, target.numel() // target.shape[-1] // n_groups


def edge_pair(nfeat, matched_nan=False):
    """1025 cells with the edge values placed by hand; returns pred, target and the four counts expected of them."""
    f32 = np.float32
    p, t = np.zeros((1025, 5), f32), np.zeros((1025, 5), f32)
    above = np.nextafter(f32(.01), f32(1.))
    #            cell   d_pred v_pred  accidentals (pred)          d_tgt  v_tgt               accidentals (target)
    cells = [(0,      1., f32(.01), (0., 1., 0.),               1., .5,               (0., 1., 0.)),   # exactly .01: off
             (1,      1., above,    (f32(.1), 0., 0.),          1., .5,               (1., 0., 0.)),   # one ulp above: on; exactly .1 is not hard
             (2,      1., NAN,      (0., 1., 0.),               1., .5,               (0., 1., 0.)),   # NaN velocity: off
             (3,      1., .5,       (0., 1., 0.),               1., -0.,              (0., 1., 0.)),   # -0.0 is no target
             (4,      1., .5,       (.3, .3, .3),               1., f32(1.4e-45),     (1., 1., 1.)),   # the smallest denormal is one
             (1023,   1., .5,       (.05, .09, 0.),             1., .5,               (0., 0., 0.)),   # all below .1 against all zero
             (1024,   5.5, .5,      (.2, .7, .1),               7., .5,               (0., 1., 0.)),   # d_tgt clamps at 6: |5.5 - 6|
             (600,    NAN, .5,      (0., 1., 0.),               0., 0.,               (0., 0., 0.))]   # NaN duration, not matched
    if matched_nan:
        cells.append((700, NAN, .5, (0., 1., 0.), 1., .5, (0., 1., 0.)))                                 # ... and matched
    for c, dp, vp, ap, dt, vt, at in cells:
        p[c] = (dp, vp) + tuple(ap)
        t[c] = (dt, vt) + tuple(at)
    assert t[4, 1] > 0 and t[4, 1] == np.frombuffer(np.int32(1).tobytes(), f32)[0] and np.signbit(t[3, 1])
    counts = dict(n_pred=6 + matched_nan, n_tgt=6 + matched_nan, tp=4 + matched_nan, acc=(3 + matched_nan) if nfeat == 5 else 0)
    return torch.from_numpy(p[:, :nfeat].copy()), torch.from_numpy(t[:, :nfeat].copy()), counts


# ---- mst_roll_metrics through the C ABI
def _offset(host, lead, device):
    """`host` on `device`, `lead` floats behind a 16-byte boundary, with the buffer it lives in."""
    buf = torch.full((host.numel() + 8,), NAN, dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[lead:lead + host.numel()]
    view.copy_(host.reshape(-1))
    assert view.data_ptr() % 16 == 4 * lead
    return view, buf


def run_metrics(native, device, pred, target, n_groups, group_cells, nfeat, lead_p=0, lead_t=0, guard=4, stream=None):
    """mst_roll_metrics into NaN-poisoned `out` and `scratch` with `guard` NaN elements either side, which must stay; the
    inputs must come back bit for bit.  Returns the records as a host (n_groups, 8) float64 tensor."""
    pred, target = torch.as_tensor(pred).reshape(-1).contiguous(), torch.as_tensor(target).reshape(-1).contiguous()
    assert pred.numel() == target.numel() == n_groups * group_cells * nfeat
    dp, pbuf = _offset(pred, lead_p, device)
    dt, tbuf = _offset(target, lead_t, device)
    p0, t0 = pbuf.cpu(), tbuf.cpu()
    nbytes = native.roll_metrics_scratch_bytes(n_groups, group_cells)
    assert nbytes == 32 * n_groups * native.roll_slices(group_cells)
    scratch = torch.full((nbytes // 8 + 2 * guard,), NAN, dtype=torch.float64, device=device)
    out = torch.full((n_groups * W + 2 * guard,), NAN, dtype=torch.float64, device=device)
    native.roll_metrics(dp.data_ptr(), dt.data_ptr(), n_groups, group_cells, nfeat, scratch.data_ptr() + 8 * guard,
                        out.data_ptr() + 8 * guard, stream if stream is not None else nat.current_stream(device))
    out, scratch = out.cpu(), scratch.cpu()
    for buf in (out, scratch):
        assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[-guard:]).all(), 'a store outside the promised range'
    assert same_bits(pbuf.cpu(), p0) and same_bits(tbuf.cpu(), t0), 'the inputs are read only'
    return out[guard:-guard].reshape(n_groups, W).clone()


def metrics_case(native, device, pred, target, n_groups, group_cells, nfeat, nontrivial=True, leads=((0, 0),)):
    want = yardstick(pred, target, n_groups, group_cells, nfeat)
    first = None
    for lead_p, lead_t in leads:
        got = run_metrics(native, device, pred, target, n_groups, group_cells, nfeat, lead_p, lead_t)
        check_records(got.numpy(), want, group_cells)
        assert first is None or same_bits(got, first)             # the same bits at every alignment
        first = got if first is None else first
    if nontrivial:
        assert counts_not_trivial(first.numpy()), first.sum(0)
    return first


def size_case(native, device, n_groups, group_cells, nfeat):
    pred, target = random_pair(n_groups * group_cells, nfeat, seed=n_groups * 7 + group_cells)
    return metrics_case(native, device, pred, target, n_groups, group_cells, nfeat, nontrivial=group_cells > 1)


def misaligned_case(native, device, nfeat):
    # an odd group_cells: with five features every second group base sits at another 16-byte phase
    pred, target = random_pair(3 * 1025, nfeat, seed=11)
    return metrics_case(native, device, pred, target, 3, 1025, nfeat, leads=((0, 0), (1, 3), (3, 1), (2, 2)))


def two_runs_case(native, device, nfeat):
    pred, target = random_pair(2 * (2 * 1024 + 777), nfeat, seed=23)
    a = run_metrics(native, device, pred, target, 2, 2 * 1024 + 777, nfeat)
    b = run_metrics(native, device, pred, target, 2, 2 * 1024 + 777, nfeat)
    assert same_bits(a, b) and counts_not_trivial(a.numpy())


def edge_case(native, device, nfeat):
    for matched_nan in (False, True):
        pred, target, counts = edge_pair(nfeat, matched_nan)
        got = run_metrics(native, device, pred, target, 1, 1025, nfeat, lead_p=1, lead_t=3).numpy()
        check_records(got, yardstick(pred, target, 1, 1025, nfeat), 1025)
        assert got[0, :5].tolist() == [1025, counts['n_pred'], counts['n_tgt'], counts['tp'], counts['acc']], got
        assert np.isnan(got[0, 6]) == matched_nan
        if not matched_nan:
            assert got[0, 6] == .5 and np.isfinite(got[0, 5])      # |5.5 - min(7, 6)|, the other matched durations are equal


def synth_case(native, device, key):
    pred, target, n_groups, group_cells = synth_pair(key)
    nfeat = target.shape[-1]
    assert group_cells % S and group_cells > S
    got = metrics_case(native, device, pred, target, n_groups, group_cells, nfeat, leads=((0, 0), (1, 3)))
    for g in range(n_groups):
        assert counts_not_trivial(got[g].numpy()), (g, got[g])
    hard_on = so.hard_output(pred.clone())[..., 1] != 0
    assert 0 < int(hard_on.sum()) < int((pred[..., 1] != 0).sum())          # the threshold does drop notes
    return got


def err_arg_case(native, device):
    lib = native.lib
    x, y = (torch.rand(10, 5) + .5).to(device), (torch.rand(10, 5) + .5).to(device)
    scratch = torch.full((8,), NAN, dtype=torch.float64, device=device)
    out = torch.full((16,), NAN, dtype=torch.float64, device=device)
    P = lambda t: t.data_ptr()
    sb = lib.mst_roll_metrics_scratch_bytes
    assert sb(1, 10) == 32 and sb(2, 1025) == 128 and sb(3, 2 ** 31 - 1) == 3 * 2 ** 21 * 32
    for n_groups, group_cells in ((0, 10), (-1, 10), (1, 0), (1, -5), (1, 2 ** 31), (2 ** 10, 2 ** 31 - 1), (2 ** 31, 1)):
        assert sb(n_groups, group_cells) <= 0, (n_groups, group_cells)
    assert sb(2 ** 10 - 1, 2 ** 31 - 1) > 0 and sb(2 ** 31 - 1, 1024) > 0
    ok = (P(x), P(y), 2, 5, 5, P(scratch), P(out))
    bad = [(0, None), (1, None), (5, None), (6, None), (4, 3), (4, 0), (4, 4), (2, 0), (2, -1), (3, 0), (3, -2), (3, 2 ** 31),
           (0, P(x) + 2), (1, P(y) + 1), (5, P(scratch) + 4), (6, P(out) + 4)]
    for at, value in bad:
        args = ok[:at] + (value,) + ok[at + 1:]
        assert lib.mst_roll_metrics(*args, None) == ERR_ARG, args
    assert lib.mst_roll_metrics(P(x), P(y), 2 ** 10, 2 ** 31 - 1, 5, P(scratch), P(out), None) == ERR_ARG     # groups x slices = 2^31
    assert torch.isnan(out).all() and torch.isnan(scratch).all()          # nothing was launched
    assert lib.mst_roll_metrics(*ok, nat.current_stream(device)) == 0
    check_records(out.cpu().numpy(), yardstick(x, y, 2, 5, 5), 5)
    assert float(out[3]) == 5 and float(out[8 + 3]) == 5                  # every cell of both groups is a matched note


# ---- mst_eval_iteration through the C ABI
PRED_NAMES = ('instruments_pred', 'mode_pred', 'bpm_pred', 'pitched_pred', 'unpitched_pred')


def eval_params(native, dims, seed=0, pitched_shift=-4.6):
    """random_params predicts every velocity near .5 — every cell "on".  Scaling the two style appliers' last Linear by 20 and
    moving their velocity bias by -4.6 spreads the velocities over (0, 1) with most cells off; checked with the oracle on the
    CPU, SMALL widths then give TP, FP and FN all > 0 on both rolls.  At FULL widths the same change leaves every pitched
    velocity below .002 (TP = FP = 0, checked the same way), so there the pitched bias moves by +10 instead, which gives
    81 / 1657 / 143 at (2, 2, 2) and 2795 / 52865 / 4423 at the bench shape: `pitched_shift`."""
    flat, named, table = pc.random_params(native, dims, seed)
    hit = 0
    for name, off, shape in table:
        n = int(np.prod(shape))
        if name.endswith('_style_applier.linear.weight'):
            flat[off:off + n] *= 20.
            hit += 1
        if name.endswith('_style_applier.linear.bias'):
            flat[off + 1] += pitched_shift if name.startswith('pitched') else -4.6
            hit += 1
    assert hit == 4, hit          # (the table lists the unpitched applier whether or not a clip has percussion)
    return flat


def _set_clip(plan, clip, k=0, ws=None):
    plan.set_inputs(mode=clip['mode'], bpm=clip['bpm'], instr=clip['instruments_features'], used=clip['used_instruments'],
                    bpm_target=float(clip['bpm_int']), ws=ws, clip=k)


def _poison(plan, ws, unp):
    """NaN into the gradient and scratch arenas and into every prediction slot: evaluation must write what it reports."""
    ws[plan.clips * plan.clip_stride:].fill_(NAN)
    for k in range(plan.clips):
        for name in PRED_NAMES[:4] + (PRED_NAMES[4:] if unp else ()):
            plan.view(name, ws=ws, clip=k).fill_(NAN)


def _run_eval(plan, params, xp, xu, clips, unp, guard=4):
    K, C = plan.clips, plan.dims.C
    ws = plan.new_ws()
    _poison(plan, ws, unp)
    for k, clip in enumerate(clips):
        _set_clip(plan, clip, k, ws)
    losses = torch.full((K, nat.N_LOSSES), -7., device=plan.device)
    buf = torch.full((K * (C + 2) * W + 2 * guard,), NAN, dtype=torch.float64, device=plan.device)
    metrics = buf[guard:-guard].view(K, C + 2, W)
    plan.eval_iteration(params, xp, xu, losses, metrics, ws=ws)
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[-guard:]).all()
    return ws, losses, metrics.clone()


def eval_case(native, device, widths, C, R, T, unp, K=1, seed=0, density=.05, **plan_opts):
    dims1, dimsK = make_dims(widths, C, R, T, unp), make_dims(widths, C, R, T, unp, clips=K)
    planK = nat.Plan(native, dimsK, device, **plan_opts)
    assert planK.clips == K
    opts1 = dict(plan_opts, gemm_tile=planK.gemm_tile)      # the bitwise comparisons need the one-clip plan on the same tiling
    params = eval_params(native, dims1, seed, -4.6 if widths['beat'] == pc.SMALL['beat'] else 10.).to(device)
    before = params.clone()
    clips = [synth_clip(5 + k, C, R, T, unp, density=density) for k in range(K)]
    xp = torch.cat([c['pitched'] for c in clips]).contiguous().to(device)
    xu = torch.cat([c['unpitched'] for c in clips]).contiguous().to(device) if unp else None
    ws, losses, metrics = _run_eval(planK, params, xp, xu, clips, unp)
    assert native.lib.mst_eval_scratch_bytes(planK.handle) == 32 * K * (C * native.roll_slices(R * T * 560) +
                                                                        (native.roll_slices(R * T * 470) if unp else 0))
    names = PRED_NAMES[:4] + (PRED_NAMES[4:] if unp else ())
    # the losses of mst_train_iteration on a second workspace with the same inputs
    wsT = planK.new_ws()
    wsT[planK.clips * planK.clip_stride:].fill_(NAN)
    for k, clip in enumerate(clips):
        _set_clip(planK, clip, k, wsT)
    lossesT = torch.full((K, nat.N_LOSSES), -7., device=device)
    planK.train_iteration(params, torch.zeros_like(params), xp, xu, lossesT, ws=wsT)
    assert same_bits(losses, lossesT), (losses, lossesT)
    assert torch.isfinite(losses[:, 0]).all()
    # the predictions of mst_forward on a third workspace
    wsF = planK.new_ws()
    for k, clip in enumerate(clips):
        _set_clip(planK, clip, k, wsF)
    planK.forward(nat.STAGE_ALL, params, xp, xu, ws=wsF)
    for k in range(K):
        for name in names:
            assert same_bits(planK.view(name, ws=ws, clip=k), planK.view(name, ws=wsF, clip=k)), (name, k)
    # the metrics: mst_roll_metrics and the numpy yardstick of the workspace's OWN predictions (a velocity within rounding of
    # .01 may fall either way between two implementations of the model, so the oracle's predictions are no yardstick)
    cells_p, cells_u = R * T * 560, R * T * 470
    total = np.zeros((2, W))
    for k, clip in enumerate(clips):
        pp = planK.view('pitched_pred', ws=ws, clip=k).clone()
        check_records(metrics[k, :C].cpu().numpy(), yardstick(pp, clip['pitched'], C, cells_p, 5), cells_p)
        assert same_bits(metrics[k, :C], run_metrics(native, device, pp, clip['pitched'], C, cells_p, 5)), k
        total[0] += metrics[k, :C].cpu().numpy().sum(0)
        if unp:
            up = planK.view('unpitched_pred', ws=ws, clip=k).clone()
            check_records(metrics[k, C].cpu().numpy(), yardstick(up, clip['unpitched'], 1, cells_u, 2), cells_u)
            assert same_bits(metrics[k, C:C + 1], run_metrics(native, device, up, clip['unpitched'], 1, cells_u, 2)), k
            total[1] += metrics[k, C].cpu().numpy()
        else:
            assert not bits(metrics[k, C]).any()                     # all zero, +0.0
        want = song_info_yardstick(*(planK.view(n, ws=ws, clip=k) for n in ('instruments_pred', 'used_instruments', 'mode_pred',
                                                                           'mode', 'bpm_pred', 'bpm_target')))
        assert np.array_equal(metrics[k, C + 1].cpu().numpy(), want), (metrics[k, C + 1], want)
        assert want[0] == dims1.n_instruments and want[2] == clip['used_instruments'].sum()
    # TP, FP and FN all > 0 on both rolls, on what the kernels predicted
    for roll in total[:2 if unp else 1]:
        tp, fp, fn = roll[3], roll[1] - roll[3], roll[2] - roll[3]
        assert tp > 0 and fp > 0 and fn > 0, (tp, fp, fn)
    # per clip, a K-clip plan matches K one-clip runs
    if K > 1:
        plan1 = nat.Plan(native, dims1, device, **opts1)
        for k, clip in enumerate(clips):
            a, b = pc.dev_clip(clip, device)
            _, losses1, metrics1 = _run_eval(plan1, params, a, b, [clip], unp)
            assert same_bits(losses1[0], losses[k]) and same_bits(metrics1[0], metrics[k]), k
    assert same_bits(params, before)
    # a second call gives the same bits
    _, losses2, metrics2 = _run_eval(planK, params, xp, xu, clips, unp)
    assert same_bits(losses2, losses) and same_bits(metrics2, metrics)
    return metrics


def eval_refusals(native, device):
    dims = make_dims(pc.SMALL, 2, 2, 1, True)
    plan = nat.Plan(native, dims, device)
    params = eval_params(native, dims).to(device)
    clip = synth_clip(5, 2, 2, 1, True)
    xp, xu = pc.dev_clip(clip, device)
    metrics = torch.full((4, W), NAN, dtype=torch.float64, device=device)
    scratch = plan.eval_scratch()
    P = lambda t: None if t is None else t.data_ptr()
    ok = (plan.handle, P(params), P(plan.ws), P(xp), P(xu), None, P(metrics), P(scratch))
    for at, value in ((0, None), (1, None), (2, None), (3, None), (4, None), (6, None), (7, None), (6, P(metrics) + 4), (7, P(scratch) + 4)):
        args = ok[:at] + (value,) + ok[at + 1:]
        assert native.lib.mst_eval_iteration(*args, None) == ERR_ARG, at
    assert torch.isnan(metrics).all()
    assert native.lib.mst_eval_scratch_bytes(None) <= 0
    tiled = nat.Plan(native, make_dims(pc.SMALL, 2, 2, 1, True), device, tile_r0=0, tile_rows=1)
    assert native.lib.mst_eval_scratch_bytes(tiled.handle) == ERR_UNSUPPORTED
    assert native.lib.mst_eval_iteration(tiled.handle, *ok[1:], None) == ERR_UNSUPPORTED
