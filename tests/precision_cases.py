"""Precision cases shared by the CPU-interpreter tests and the -m gpu tests: the HIP kernels against the oracle evaluated in
FLOAT64 (parameters and clip tensors cast to double; the oracle's code is dtype-agnostic), with the fp32 oracle run beside
it as the yardstick of what fp32 can resolve at all.  Every assertion here is against float64, never against another fp32
evaluation: that is what lets the project bar (pc.TOL) apply to every one of the parameter gradient tensors, the tiny ones
included, where parity_cases.oracle_case has to fall back to a loose structural guard."""
import contextlib
import math

import numpy as np
import torch

import parity_cases as pc
from oracle import style_oracle as so
from tools.synth import synth_clip
from simutil import make_dims, rel
from style import _native as nat

TOL = pc.TOL
REF_TOL = TOL / 8       # a case is admitted only if the fp32 oracle itself is this close to float64 on every tensor
FLOOR = 1e-6            # denominator floor of the per-tensor measure, as a share of the whole gradient's norm
LEAF_TOL = 2e-5         # loss leaves: |got - ref| <= LEAF_TOL * max(1, |ref|), as in pc.loss_normalize_case
BOUNDARY = ('style', 'melody', 'rhythm')


class _Mids(dict):
    """`mids=` of so.iteration: the stage-boundary tensors keep their .grad (iteration calls backward itself)."""

    def update(self, *a, **kw):
        super().update(*a, **kw)
        for k in BOUNDARY:
            if k in kw:
                kw[k].retain_grad()


def _double_clip(clip):
    return {k: (v.double() if torch.is_tensor(v) else v) for k, v in clip.items()}


def _flat_grad(named, table):
    return torch.cat([(named[n].grad if named[n].grad is not None else torch.zeros_like(named[n])).reshape(-1)
                      for n, _, _ in table]).double().numpy()


@contextlib.contextmanager
def _one_thread():
    """The fp32 yardstick on one thread: torch's fp32 reductions over the note rows depend on how many threads share them
    (melody_size 16 at (C, R, T) = (2, 8, 4): melody_encoder.linear.weight is at 5e-5 ... 1e-4 of float64 for every seed on
    16 threads of one host and at 1e-6 on one thread), and the reference condition must not depend on the host's thread count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


_oracle_cache = {}


def oracle_runs(native, widths, C, R, T, unp, K, density, lstm_scale, seed):
    """Parameters, clips and the two oracle runs (fp32, float64) of a case: computed once per set of inputs and shared by
    every plan variant that is tested on them; nothing in the result is written to afterwards."""
    key = (tuple(sorted(widths.items())), C, R, T, bool(unp), K, density, lstm_scale, seed)
    if key in _oracle_cache:
        return _oracle_cache[key]
    dims = make_dims(widths, C, R, T, unp)
    flat, named, table = pc.random_params(native, dims, seed)
    if lstm_scale != 1.0:
        with torch.no_grad():
            for name, off, shape in table:
                if 'lstm' in name:
                    n = int(np.prod(shape))
                    flat[off:off + n] *= lstm_scale
                    named[name].copy_(flat[off:off + n].view(*shape))
    named64 = {n: t.detach().double().requires_grad_(True) for n, t in named.items()}
    clips = [synth_clip(5 + k, C, R, T, unp, density=density) for k in range(K)]
    mids64, out64, losses64 = [], [], []
    for clip in clips:
        with _one_thread():
            so.iteration(named, clip, mids=_Mids())
        m = _Mids()
        (info, xp, xu), leaves = so.iteration(named64, _double_clip(clip), mids=m)
        m.update(pitched_pred=xp, instruments_pred=info[0], mode_pred=info[1], bpm_pred=info[2])
        if unp:
            m.update(unpitched_pred=xu)
        out64.append({k: v.detach().numpy() for k, v in m.items()})
        mids64.append({k: m[k].grad.numpy() for k in BOUNDARY})
        losses64.append(leaves)
    res = dict(flat=flat, table=table, clips=clips, g32=_flat_grad(named, table), g64=_flat_grad(named64, table), out64=out64,
               bgrad64=mids64, losses64=losses64)
    _oracle_cache[key] = res
    return res


def tensor_errors(table, g64, x):
    """e(x, t) = ||x_t - g64_t|| / max(||g64_t||, FLOOR * ||g64||) for every parameter tensor t, with the tensor's share."""
    whole = float(np.linalg.norm(g64))
    out = []
    for name, off, shape in table:
        n = int(np.prod(shape))
        r = g64[off:off + n]
        nr = float(np.linalg.norm(r))
        out.append((name, nr / whole, float(np.linalg.norm(x[off:off + n] - r)) / max(nr, FLOOR * whole)))
    return out


def top_share(table, g64, x, name):
    """Share of the largest single element in ||x_t - g64_t||^2 of tensor `name`: near 1 when one unit sits on the other side of
    a kink than in float64, small when a term is missing or mis-scaled."""
    off, shape = next((off, shape) for n, off, shape in table if n == name)
    d = (x[off:off + int(np.prod(shape))] - g64[off:off + int(np.prod(shape))]) ** 2
    return float(d.max() / max(d.sum(), 1e-300))


def precise_case(native, device, widths, C, R, T, unp, *, K=1, density, lstm_scale=1.0, seed=0, tag=None, **plan_opts):
    """One train iteration of a K-clip plan against the float64 oracle: every parameter gradient tensor, the activations, the
    stage-boundary gradients and the loss leaves.  Returns the table [(name, share, e_o, e_k)] over all parameter tensors.
    With `tag` the figures of report() are printed before anything is asserted on the kernels, so a failing case shows them too.
    `seed` draws the parameters: an fp32 evaluation (the yardstick's or the kernels') can put a leaky-ReLU pre-activation or a
    min / relu argument of the loss on the other side of its kink than float64 does, which shows as ONE element of one bias
    gradient (and of the weights fed by the same unit) off by ~1e-8 absolute while every other element agrees to 1e-11 - a
    property of the draw, not a dropped term; the failure messages carry the share of the largest single element for that."""
    o = oracle_runs(native, widths, C, R, T, unp, K, density, lstm_scale, seed)
    table, clips, g64 = o['table'], o['clips'], o['g64']
    # ---- conditions on the case itself: fp32 can resolve it, and (scaled LSTMs) it really left the linear regime
    e_o = tensor_errors(table, g64, o['g32'])
    worst_o = max(e_o, key=lambda r: r[2])
    assert worst_o[2] <= REF_TOL, ('reference condition: the fp32 oracle is too far from float64; largest single element\'s share '
                                   'of the squared difference (near 1: a unit flipped at a kink, take another seed)',
                                   worst_o, top_share(table, g64, o['g32'], worst_o[0]))
    if lstm_scale > 1:
        p99 = lambda key: float(np.percentile(np.abs(np.concatenate([m[key].reshape(-1) for m in o['out64']])), 99))
        assert p99('pitched_beats') >= 0.25, ('saturation condition', 'pitched_beats', p99('pitched_beats'))
        if unp:
            assert p99('unpitched_beats') >= 0.4, ('saturation condition', 'unpitched_beats', p99('unpitched_beats'))
    # ---- the kernels: one K-clip plan, NaN-poisoned arenas
    plan = nat.Plan(native, make_dims(widths, C, R, T, unp, clips=K), device, **plan_opts)
    assert plan.clips == K
    for k, clip in enumerate(clips):
        plan.set_inputs(mode=clip['mode'], bpm=clip['bpm'], instr=clip['instruments_features'], used=clip['used_instruments'],
                        bpm_target=float(clip['bpm_int']), clip=k)
    xp = torch.cat([c['pitched'] for c in clips]).contiguous().to(device)
    xu = torch.cat([c['unpitched'] for c in clips]).contiguous().to(device) if unp else None
    params = o['flat'].to(device)
    gparams = torch.zeros_like(params)
    losses = torch.zeros(K, nat.N_LOSSES, device=device)
    pc.poison(plan)
    plan.train_iteration(params, gparams, xp, xu, losses)
    gk = gparams.cpu().double().numpy()
    e_k = tensor_errors(table, g64, gk)
    result = [(n, share, eo, ek) for (n, share, eo), (_, _, ek) in zip(e_o, e_k)]
    if tag:
        report(tag, result)
    # ---- activations, stage-boundary gradients, loss leaves: per clip
    slots = ['pitched_beats', 'pitched_bars', 'pitched_rhythm', 'style', 'melody', 'rhythm', 'pitched_pred', 'instruments_pred',
             'mode_pred', 'bpm_pred'] + (['unpitched_beats', 'unpitched_bars', 'unpitched_rhythm', 'unpitched_pred'] if unp else [])
    lc = losses.cpu()
    bad = []
    for k in range(K):
        for s in slots:
            e = rel(plan.view(s, clip=k).cpu().numpy(), o['out64'][k][s])
            if not e <= TOL:
                bad.append(('activation', k, s, e))
        for s in BOUNDARY:
            e = rel(plan.grad(s, clip=k).cpu().numpy(), o['bgrad64'][k][s])
            if not e <= TOL:
                bad.append(('stage-boundary gradient', k, s, e))
        ref = o['losses64'][k]
        for i, key in enumerate(nat.LOSS_KEYS):
            got = float(lc[k, i])
            if key in ref:
                if not abs(got - ref[key]) <= LEAF_TOL * max(1., abs(ref[key])):
                    bad.append(('loss leaf', k, key, got, ref[key]))
            elif not math.isnan(got):
                bad.append(('loss leaf of an absent pair is not NaN', k, key, got))
    bad += [('parameter gradient', n, 'share', share, 'e_o', eo, 'e_k', ek, 'largest single element of the squared difference',
             top_share(table, g64, gk, n)) for n, share, eo, ek in result if not ek <= TOL]
    assert not bad, bad
    return result


def report(tag, table):
    """The figures DESIGN.md records for a case: the five worst tensors, max e_k and the largest e_k / max(e_o, median e_o)
    (recorded, not asserted)."""
    med = float(np.median([r[2] for r in table]))
    ratio = max(table, key=lambda r: r[3] / max(r[2], med))
    print(f'{tag}: max e_o {max(r[2] for r in table):.2e} max e_k {max(r[3] for r in table):.2e} '
          f'largest ratio {ratio[3] / max(ratio[2], med):.1f} ({ratio[0]})')
    for name, share, eo, ek in sorted(table, key=lambda r: -r[3])[:5]:
        print(f'    {name}: share {share:.1e} e_o {eo:.2e} e_k {ek:.2e}')


# ---------------------------------------------------------------- loss edges
def _note_tensors(g, n, nacc, density, dur_max=4.0):
    """(prediction, target) of n positions: the target like tools.synth._roll, the prediction random in the output ranges of
    the appliers (duration in [0, 6], everything else in [0, 1])."""
    mask = (torch.rand(n, generator=g) < density).float()
    feats = [torch.rand(n, generator=g) * dur_max * mask, (0.1 + 0.9 * torch.rand(n, generator=g)) * mask]
    which = torch.randint(0, max(nacc, 1), (n,), generator=g)
    feats += [(which == a).float() * mask for a in range(nacc)]
    target = torch.stack(feats, -1).contiguous()
    pred = torch.rand(n, 2 + nacc, generator=g)
    pred[:, 0] *= 6.0
    return pred.contiguous(), target


def _loss_inputs(seed, n_p=1123, n_u=1057, density=0.1, dur_max=4.0):
    g = torch.Generator().manual_seed(seed)
    pp, pt = _note_tensors(g, n_p, 3, density, dur_max)
    up, ut = _note_tensors(g, n_u, 0, density, dur_max)
    it = (torch.rand(1, 41, generator=g) < 0.2).float()
    return dict(pp=pp, pt=pt, up=up, ut=ut, il=torch.randn(1, 41, generator=g), it=it, ml=torch.randn(1, 2, generator=g),
                mt=torch.tensor([[0., 1.]]), bp=torch.tensor([131.5]), bt=torch.tensor([120.]))


def loss_edge_inputs(large=True):
    """[(name, inputs, normalize values)]: every branch of mst_total_loss_fwd / _bwd that the loss_normalize fixture leaves
    untaken.  `large` includes the case beyond LOSS_MAXBLK workgroups x 1024 positions."""
    cases = [('baseline', _loss_inputs(1), (0, 1))]
    cases.append(('durations up to 12: the clamp at 6 is active', _loss_inputs(2, dur_max=12.0), (0, 1)))
    # ties of predicted and target velocity on every second position (torch.min splits the gradient), accidentals equal to the
    # one-hot target — exactly 0 / 1 — on every third
    x = _loss_inputs(3)
    x['pp'][::2, 1] = x['pt'][::2, 1]
    x['up'][::2, 1] = x['ut'][::2, 1]
    x['pp'][::3, 2:] = x['pt'][::3, 2:]
    cases.append(('ties and saturated accidentals', x, (0, 1)))
    # p = 1 against t = 0 and p = 0 against t = 1 on sounding positions: the -100 clamp of the logs, the 1e-12 clamp of the
    # backward.  normalize = 0 only: the fp32 tanh of a loss of this size is exactly 1 and its derivative exactly 0 where
    # float64 keeps ~1e-10 — an artefact of the comparison, not of the kernel
    y = {k: v.clone() for k, v in x.items()}
    sounding = torch.nonzero(y['pt'][:, 1] > 0).reshape(-1)[:6]
    assert len(sounding) == 6
    y['pp'][sounding, 2:] = 1.0 - y['pt'][sounding, 2:]
    cases.append(('accidentals at the log clamps', y, (0,)))
    x = _loss_inputs(4)
    x['pp'][:, 1] = 0.
    x['up'][:, 1] = 0.
    cases.append(('all predicted velocities 0: safe_div epsilon branches, notes loss 1', x, (0, 1)))
    x = _loss_inputs(5)
    x['pp'] = x['pt'].clone()
    x['pp'][:, 2:].clamp_(1e-3, 1 - 1e-3)
    x['up'] = x['ut'].clone()
    cases.append(('prediction equal to the target', x, (0, 1)))
    x = _loss_inputs(6)
    x['il'] *= 60.
    x['ml'] *= 80.
    x['bp'] = torch.tensor([200.])
    x['up'] = x['ut'] = None
    cases.append(('large logits, bpm 200, no unpitched pair', x, (0, 1)))
    if large:
        x = _loss_inputs(7, n_p=256 * 1024 + 777, n_u=3, density=0.02)
        x['ut'][:, 0] = torch.tensor([0.5, 3.0, 7.0])
        x['ut'][:, 1] = torch.tensor([0.9, 0.2, 0.6])
        cases.append(('grid wrap, ragged last tile, a tensor smaller than a tile', x, (0, 1)))
    x = _loss_inputs(8)
    x['ut'].zero_()
    cases.append(('unpitched target all silent: 0 / 0 masked means', x, (0, 1)))
    return cases


def _loss_reference(x, normalize):
    """so.total_loss and autograd in float64 on the same fp32-VALUED inputs (cast after they were built in fp32, so exact
    0, 1 and ties are the same on both sides)."""
    d = {k: (None if v is None else v.double()) for k, v in x.items()}
    leaves = [k for k in ('pp', 'up', 'il', 'ml', 'bp') if d[k] is not None]
    for k in leaves:
        d[k].requires_grad_(True)
    out = so.total_loss(d['il'], d['it'], d['bp'], d['bt'], d['ml'], d['mt'], d['pp'], d['pt'], d['up'], d['ut'], normalize=bool(normalize))
    out['total'].backward()
    return {k: float(v.detach()) for k, v in out.items()}, {k: d[k].grad.numpy().reshape(-1) for k in leaves}


def loss_edge_case(native, device, large=True):
    lib, P = native.lib, nat.ptr
    stream = nat.current_stream(device)
    bad = []
    for name, x, normalizes in loss_edge_inputs(large):
        dx = {k: (None if v is None else v.contiguous().to(device)) for k, v in x.items()}
        n_p, n_u = x['pp'].shape[0], (0 if x['up'] is None else x['up'].shape[0])
        for normalize in normalizes:
            ref_leaves, ref_grads = _loss_reference(x, normalize)
            losses = torch.full((nat.N_LOSSES,), -7., device=device)
            saved = torch.full((nat.LOSS_SAVED,), float('nan'), device=device)
            scratch = torch.full((lib.mst_loss_scratch_floats(),), float('nan'), device=device)
            nat.check(lib.mst_total_loss_fwd(P(dx['pp']), P(dx['pt']), n_p, P(dx['up']), P(dx['ut']), n_u, P(dx['il']), P(dx['it']), 41,
                                             P(dx['ml']), P(dx['mt']), P(dx['bp']), P(dx['bt']), normalize, P(losses), P(saved), P(scratch),
                                             stream), 'mst_total_loss_fwd')
            gl = torch.zeros(nat.N_LOSSES, device=device)
            gl[0] = 1.
            got = {k: torch.full_like(dx[k], float('nan')) for k in ref_grads}
            nat.check(lib.mst_total_loss_bwd(P(dx['pp']), P(dx['pt']), n_p, P(dx['up']), P(dx['ut']), n_u, P(dx['il']), P(dx['it']), 41,
                                             P(dx['ml']), P(dx['mt']), P(dx['bp']), P(dx['bt']), P(saved), P(gl), P(got['pp']), P(got.get('up')),
                                             P(got['il']), P(got['ml']), P(got['bp']), stream), 'mst_total_loss_bwd')
            lc = losses.cpu()
            for i, key in enumerate(nat.LOSS_KEYS):
                g, r = float(lc[i]), ref_leaves.get(key, float('nan'))
                if math.isnan(r) != math.isnan(g) or (not math.isnan(r) and not abs(g - r) <= LEAF_TOL * max(1., abs(r))):
                    bad.append((name, normalize, 'leaf', key, g, r))
            largest = max(float(np.linalg.norm(np.nan_to_num(r))) for r in ref_grads.values())
            for k, r in ref_grads.items():
                g = got[k].cpu().double().numpy().reshape(-1)
                if not np.array_equal(np.isnan(g), np.isnan(r)):
                    bad.append((name, normalize, 'gradient NaN mask', k, int(np.isnan(g).sum()), int(np.isnan(r).sum())))
                    continue
                err = float(np.linalg.norm(np.nan_to_num(g) - np.nan_to_num(r)))
                bound = TOL * max(float(np.linalg.norm(np.nan_to_num(r))), FLOOR * largest)
                if not err <= bound:
                    bad.append((name, normalize, 'gradient', k, err, bound))
    assert not bad, bad


# ---------------------------------------------------------------- Adam + StepLR
ADAM_SIZES = (1, 255, 1025, 2 * 2048 * 256 + 7)       # the last one wraps the grid cap of 2048 workgroups x 256 lanes


def adam_schedule_case(native, device, sizes=ADAM_SIZES):
    """mst_adam_step and mst_adam_step2 over 8 steps against torch.optim.Adam(lr=.01) + StepLR(step_size=3, gamma=.5) in
    float64: the schedule crosses two boundaries.  torch's own fp32 Adam runs beside it as the yardstick."""
    lr0, b1, b2, eps, step_size, gamma, steps = .01, .9, .999, 1e-8, 3, .5, 8
    stream = nat.current_stream(device)
    for n in sizes:
        for two in (False, True):
            g = torch.Generator().manual_seed(n + int(two))
            p0 = torch.randn(n, generator=g)
            p64, p32 = p0.double().requires_grad_(True), p0.clone().requires_grad_(True)
            refs = []
            for p in (p64, p32):
                opt = torch.optim.Adam([p], lr=lr0, betas=(b1, b2), eps=eps)
                refs.append((p, opt, torch.optim.lr_scheduler.StepLR(opt, step_size=step_size, gamma=gamma)))
            pk = p0.clone().to(device)
            m, v, state = torch.zeros_like(pk), torch.zeros_like(pk), torch.zeros(4, device=device)
            idx = torch.arange(n)
            for t in range(1, steps + 1):
                # N(0, 1e-2) with exact zeros (fixed positions: 0 / (0 + eps) from the first step on; random ones: decaying
                # moments) and elements at 1e-12, where eps dominates the denominator
                grad = torch.randn(n, generator=g) * 1e-2
                grad[torch.rand(n, generator=g) < 0.05] = 0.
                grad[idx % 7 == 3] = 0.
                grad[idx % 11 == 5] = 1e-12
                for p, opt, sched in refs:
                    p.grad = grad.to(p.dtype)
                    opt.step()
                    sched.step()
                zero_grad = t % 2
                if two:       # both halves sum to the gradient exactly in fp32: whole / nothing / half
                    sel = idx % 3
                    ga = torch.where(sel == 0, grad, torch.where(sel == 1, torch.zeros_like(grad), grad * 0.5))
                    bufs = [ga.to(device), (grad - ga).to(device)]
                    assert torch.equal(ga + (grad - ga), grad)
                    nat.check(native.lib.mst_adam_step2(nat.ptr(pk), nat.ptr(bufs[0]), nat.ptr(bufs[1]), nat.ptr(m), nat.ptr(v), n,
                                                        nat.ptr(state), lr0, b1, b2, eps, step_size, gamma, zero_grad, stream), 'adam2')
                else:
                    bufs = [grad.to(device)]
                    nat.check(native.lib.mst_adam_step(nat.ptr(pk), nat.ptr(bufs[0]), nat.ptr(m), nat.ptr(v), n, nat.ptr(state),
                                                       lr0, b1, b2, eps, step_size, gamma, zero_grad, stream), 'adam')
                ref = p64.detach()
                e_o = float((p32.detach().double() - ref).abs().max())
                e_k = float((pk.cpu().double() - ref).abs().max())
                bound = max(8 * e_o, 4 * 2.0 ** -24 * float(ref.abs().max()))
                assert e_k <= bound, ('parameters', n, two, t, e_k, e_o, bound)
                st = state.cpu()
                assert float(st[0]) == t, ('step count', n, two, t, float(st[0]))
                want = lr0 * gamma ** ((t - 1) // step_size) / (1 - b1 ** t)
                assert abs(float(st[1]) - want) <= 1e-6 * want, ('lr_t / (1 - beta1^t)', n, two, t, float(st[1]), want)
                for b, orig in zip(bufs, [grad] if not two else [ga, grad - ga]):
                    if zero_grad:
                        assert float(b.abs().max()) == 0., ('zero_grad', n, two, t)
                    else:
                        assert torch.equal(b.cpu(), orig), ('gradient kept', n, two, t)
