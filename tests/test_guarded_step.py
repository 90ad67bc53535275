"""Guarded optimizer step on the CPU interpreter: the global gradient norm (mst_grad_norm), clipping as "scale, then the
existing step" bit for bit, the skip of a non-finite step, per-tensor norms (mst_grad_norms), argument checks, and the
host-side Python of FusedAdam / train() / LossLog that needs no GPU."""
import csv
import io

import numpy as np
import pytest
import torch

import guard_cases as gc
from simutil import sim_native


@pytest.fixture(scope='module')
def lib():
    return sim_native().lib


@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('two', [False, True])
@pytest.mark.parametrize('n', gc.SIZES)
def test_norm_is_within_one_ulp_and_reproducible(lib, n, two, lead):
    # the double sum's relative error is at most n * 2^-53, far below 2^-24: only the final rounding can differ
    b = gc.Bufs(lib, n, two=two, lead=lead)
    g, g2 = gc.mixed(n, 1), (gc.mixed(n, 2) if two else None)
    b.set_grads(g, g2)
    got, again = b.norm(), b.norm()
    want = gc.arbiter_norm(g, g2)
    print(n, two, lead, got, want, gc.ulps(got, want))
    assert gc.ulps(got, want) <= 1
    assert got.view(np.int32) == again.view(np.int32)


def test_phase_mismatch_between_the_two_buffers_takes_scalar_loads(lib):
    n = 4099
    b = gc.Bufs(lib, n, two=True)
    g, g2 = gc.mixed(n, 1), gc.mixed(n, 2)
    b.set_grads(g, g2)
    aligned = b.norm()
    shifted = torch.zeros(n + 8)
    b.g2 = shifted[1:1 + n]
    b.g2.copy_(torch.from_numpy(g2))
    assert gc.ulps(b.norm(), gc.arbiter_norm(g, g2)) <= 1 and gc.ulps(aligned, gc.arbiter_norm(g, g2)) <= 1


def test_small_case_equals_torch_clip_grad_norm(lib):
    b = gc.Bufs(lib, 2)
    b.set_grads([3., 4.])
    assert b.guarded(2.5, 0, 0) == 0
    guard = b.guard.numpy()
    assert guard[0] == 5. and guard[4] == 1
    q = torch.nn.Parameter(torch.zeros(2))
    q.grad = torch.tensor([3., 4.])
    total = torch.nn.utils.clip_grad_norm_([q], 2.5)
    assert float(total) == 5.
    scaled = torch.tensor([3., 4.]) * torch.tensor(guard[1])
    assert gc.same_bits(scaled, q.grad), (scaled, q.grad)


@pytest.mark.parametrize('two', [False, True])
@pytest.mark.parametrize('n', gc.SIZES)
def test_clip_is_scale_then_the_existing_step_bitwise(lib, n, two):
    gc.check_clip_is_scale_then_step(lib, n, 'cpu', two)


@pytest.mark.parametrize('max_norm', [0., -1., gc.INF])
@pytest.mark.parametrize('two', [False, True])
def test_guard_off_is_the_old_step(lib, two, max_norm):
    n = 4099
    a = gc.Bufs(lib, n, two=two, seed=3)
    b = a.clone()
    for k in range(2):
        g, g2 = gc.mixed(n, 30 + k), (gc.mixed(n, 40 + k) if two else None)
        a.set_grads(g, g2)
        b.set_grads(g, g2)
        assert a.guarded(max_norm, 0) == 0 and b.plain() == 0
        assert a.same_optimizer(b)
        assert float(a.guard[1]) == 1 and float(a.guard[4]) == 0 and gc.ulps(a.guard[0].item(), gc.arbiter_norm(g, g2)) <= 1


CASES = {name: (g, g2) for n in (1025, 4099) for name, g, g2 in ((f'{c[0]}-{n}', c[1], c[2]) for c in gc.nonfinite_cases(n))}


@pytest.mark.parametrize('zero_grad', [0, 1])
@pytest.mark.parametrize('name', sorted(CASES))
def test_nonfinite_step_is_skipped(lib, name, zero_grad):
    g, g2 = CASES[name]
    assert not np.isfinite(gc.arbiter_norm(g, g2))
    gc.check_skip(lib, len(g), 'cpu', name, g, g2, zero_grad)


@pytest.mark.parametrize('two', [False, True])
def test_per_tensor_norms(lib, two):
    lengths = [1, 2, 255, 257, 70000]
    offsets, at = [], 1
    for ln in lengths:                      # odd offsets, gaps between the tensors
        offsets.append(at)
        at += ln + (2 if ln % 2 else 3)
    g, g2 = gc.mixed(at, 5), (gc.mixed(at, 6) if two else None)
    tg, tg2 = torch.from_numpy(g), (torch.from_numpy(g2) if two else None)
    off, ln = torch.tensor(offsets, dtype=torch.int64), torch.tensor(lengths, dtype=torch.int64)
    out = torch.zeros(len(lengths))
    assert lib.mst_grad_norms(tg.data_ptr(), tg2.data_ptr() if two else None, off.data_ptr(), ln.data_ptr(), len(lengths),
                              out.data_ptr(), None) == 0
    for k, (o, l) in enumerate(zip(offsets, lengths)):
        want = gc.arbiter_norm(g[o:o + l], g2[o:o + l] if two else None)
        assert gc.ulps(out[k].item(), want) <= 1, (k, out[k].item(), want)


def test_bad_arguments_return_err_arg(lib):
    n = 16
    b = gc.Bufs(lib, n, two=True)
    P = lambda t: t.data_ptr()
    assert lib.mst_grad_guard_scratch_bytes(0) <= 0 and lib.mst_grad_guard_scratch_bytes(-5) <= 0
    assert lib.mst_grad_guard_scratch_bytes(4096) == 8 and lib.mst_grad_guard_scratch_bytes(4097) == 16
    out = torch.zeros(1)
    sc = P(b.scratch)
    assert lib.mst_grad_norm(None, None, n, sc, P(out), None) == gc.ERR_ARG
    assert lib.mst_grad_norm(P(b.g), None, 0, sc, P(out), None) == gc.ERR_ARG
    assert lib.mst_grad_norm(P(b.g), None, n, None, P(out), None) == gc.ERR_ARG
    assert lib.mst_grad_norm(P(b.g), None, n, sc, None, None) == gc.ERR_ARG
    i64 = torch.zeros(2, dtype=torch.int64)
    assert lib.mst_grad_norms(None, None, P(i64), P(i64), 1, P(out), None) == gc.ERR_ARG
    assert lib.mst_grad_norms(P(b.g), None, None, P(i64), 1, P(out), None) == gc.ERR_ARG
    assert lib.mst_grad_norms(P(b.g), None, P(i64), None, 1, P(out), None) == gc.ERR_ARG
    assert lib.mst_grad_norms(P(b.g), None, P(i64), P(i64), 0, P(out), None) == gc.ERR_ARG
    assert lib.mst_grad_norms(P(b.g), None, P(i64), P(i64), 1, None, None) == gc.ERR_ARG
    good = [P(b.p), P(b.g), P(b.g2), P(b.m), P(b.v), n, P(b.state), P(b.guard), sc]
    call = lambda args, hyper=gc.HYPER, max_norm=1.: lib.mst_adam_step_guarded(*args, *hyper, max_norm, 1, 1, None)
    for i in (0, 1, 3, 4, 6, 7, 8):                      # every pointer but grads2
        bad = list(good)
        bad[i] = None
        assert call(bad) == gc.ERR_ARG, i
    assert call(good[:5] + [0] + good[6:]) == gc.ERR_ARG                     # n
    assert call(good, hyper=gc.HYPER[:4] + (0, .9)) == gc.ERR_ARG            # step_size
    assert call(good, max_norm=float('nan')) == gc.ERR_ARG
    assert call(good[:8] + [sc + 4]) == gc.ERR_ARG                           # scratch not 8-byte aligned
    assert float(b.state[0]) == 0 and not b.guard.any()                      # nothing ran
    without_g2 = list(good)
    without_g2[2] = None
    assert call(without_g2) == 0 and float(b.state[0]) == 1


# ---- host-only Python: the model is built on the CPU as tests/test_host_surface.py builds it; the flat buffers the GPU path
# would create are stood in for by CPU tensors and the binding by the interpreter build of the same sources
@pytest.fixture
def cpu_model(monkeypatch):
    from test_host_surface import SMALL, build_model
    from style import _native
    model = build_model(SMALL, seed=2)
    monkeypatch.setattr(_native, '_native', sim_native())
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()
    offs, at = [], 0
    for p in model.parameters():
        offs.append(at)
        at += p.numel()
    model._flat, model._gflat, model._offsets = flat, torch.zeros_like(flat), offs
    monkeypatch.setattr(type(model), '_sync_flat', lambda self: None)
    return model


def test_fused_adam_guarded_step_and_state_dict_roundtrip(cpu_model):
    from style.optim import FusedAdam
    plain = FusedAdam(cpu_model)
    assert plain.guard is None and plain._scratch is None and plain.guard_stats() is None      # guard off: nothing new allocated
    n = cpu_model._flat.numel()
    opt = FusedAdam(cpu_model, max_grad_norm=.5, skip_nonfinite=True)
    start = cpu_model._flat.clone()
    cpu_model._gflat.copy_(torch.from_numpy(gc.mixed(n, 3) * np.float32(1e-14)))
    g = cpu_model._gflat.clone()
    opt.step()
    stats = opt.guard_stats()
    assert stats['steps_clipped'] == 1 and stats['steps_skipped'] == 0 and 0 < stats['coef'] < 1 and not stats['skipped']
    assert gc.ulps(stats['norm'], gc.arbiter_norm(g.numpy())) <= 1 and stats['largest_norm'] == stats['norm']
    assert not cpu_model._gflat.any() and not torch.equal(cpu_model._flat, start)
    norms = None
    cpu_model._gflat.copy_(g)
    norms = opt.grad_norms()
    assert list(norms) == list(cpu_model.state_dict())
    for (name, p), off in zip(cpu_model.named_parameters(), cpu_model._offsets):
        assert gc.ulps(norms[name], gc.arbiter_norm(g.numpy()[off:off + p.numel()])) <= 1, name
    cpu_model._gflat[5] = float('nan')
    moved = cpu_model._flat.clone()
    opt.step()
    stats = opt.guard_stats()
    assert stats['skipped'] and stats['steps_skipped'] == 1 and torch.equal(cpu_model._flat, moved) and float(opt.state[0]) == 1
    # round trip through a file, bit for bit, into a fresh optimizer
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=False)
    fresh = FusedAdam(cpu_model, lr=.5)
    fresh.load_state_dict(sd)
    for k in ('exp_avg', 'exp_avg_sq', 'state', 'guard'):
        assert gc.same_bits(getattr(fresh, k), getattr(opt, k)), k
    assert (fresh.lr, fresh.betas, fresh.eps, fresh.step_size, fresh.gamma, fresh.max_grad_norm, fresh.skip_nonfinite) == \
        (opt.lr, opt.betas, opt.eps, opt.step_size, opt.gamma, .5, True)
    again = fresh.state_dict()
    assert all(gc.same_bits(again[k], sd[k]) for k in ('exp_avg', 'exp_avg_sq', 'state', 'guard')) and again['hyper'] == sd['hyper']
    wrong = dict(sd, exp_avg=torch.zeros(n + 1))
    with pytest.raises(ValueError, match='elements'):
        fresh.load_state_dict(wrong)
    with pytest.raises(ValueError):
        FusedAdam(cpu_model, max_grad_norm=float('nan'))


def test_train_refuses_guard_arguments_beside_an_optimizer(cpu_model):
    from style.train import train
    from style.optim import FusedAdam
    opt = FusedAdam(cpu_model)
    with pytest.raises(ValueError, match='optimizer'):
        train(cpu_model, iter(()), n_iterations=0, optimizer=opt, max_grad_norm=1.)
    with pytest.raises(ValueError, match='optimizer'):
        train(cpu_model, iter(()), n_iterations=0, optimizer=opt, skip_nonfinite=True)
    # without them the caller's optimizer is taken as it is (no iterations: nothing touches a GPU)
    assert train(cpu_model, iter(()), n_iterations=0, optimizer=opt, progress=False, save_path=None) is cpu_model


def test_loss_log_tolerates_nan_only_when_told(tmp_path):
    from style.train import CSV_FIELDS, LossLog
    good = torch.arange(15, dtype=torch.float32)
    bad = torch.full((15,), float('nan'))
    path = str(tmp_path / 'training.csv')
    log = LossLog(path, None, flush_every=2, tolerate_nan=True)
    log.add(0, good)
    log.add(1, bad)
    rows = list(csv.DictReader(open(path)))
    assert list(rows[0].keys()) == CSV_FIELDS and [r['iteration'] for r in rows] == ['0', '1']
    assert rows[0]['total'] == '0.0' and rows[1]['total'] == 'nan' and rows[1]['song_info_loss_total'] == ''
    strict = LossLog(str(tmp_path / 'strict.csv'), None, flush_every=1)
    with pytest.raises(AssertionError, match='NaN'):
        strict.add(0, bad)
    # the guard's figures reach the progress meter at the flush, un-averaged
    from style.utils.misc import ProgressBar
    bar = ProgressBar(None)
    bar.pbar = None
    shown = LossLog(None, bar, flush_every=1, tolerate_nan=True, guard_stats=lambda: dict(norm=3.5, steps_skipped=2))
    shown.add(0, good)
    shown.add(1, bad)
    assert bar['grad_norm'] == 3.5 and bar['skipped'] == 2. and bar['total_loss'] == 0.
