"""-m gpu: windowed batches on an MI355X.  mst_clip_window (the cases of tests/window_cases.py on the gfx950 build),
StyleTransferModel.train_windows against the batched plan fed host-cropped dense clips (same plan, same input bits: same bits)
and against one-clip passes, its hipGraph replay with other windows, its independence of the accumulation lanes, and
style.train.train(batch_clips=...)."""
import csv

import numpy as np
import pytest
import torch

import parity_cases as pc
import window_cases as wc
from simutil import make_dims, rel
from test_host_surface import build_model
from tools.synth import synth_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C, T, BARS = 2, 2, 2
SONG_BARS = (2, 5, 3, 4, 3)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('case', wc.CASES, ids=[c.__name__[5:] for c in wc.CASES])
def test_clip_window(case):
    from style import _native
    case(_native.get(), DEV)
    torch.cuda.synchronize()


# ---- train_windows
_songs = []


def songs():
    """Five songs of 2 to 5 bars (C = 2, T = 2, with percussion), each with its own mode, bpm and instruments."""
    if not _songs:
        for k, R in enumerate(SONG_BARS):
            clip = synth_clip(300 + k, C, R, T, True, density=.05, bpm=80 + 11 * k)
            if k % 2:
                clip['mode'] = torch.tensor([[0., 1.]])
            feats = torch.zeros_like(clip['instruments_features'])
            for c in range(C):
                feats[0, c, (3 * k + c) % 40] = 1.
                feats[0, c, 40 + (k + c) % 11] = 1.
            clip['instruments_features'] = feats
            _songs.append(clip)
    return _songs


def make_store():
    from style.data import SongStore, SparseClip, sparsify
    store = SongStore(DEV, capacity=256)
    for clip in songs():
        store.add(SparseClip(clip['mode'], clip['bpm'], sparsify(clip['pitched']), clip['instruments_features'],
                             sparsify(clip['unpitched']), bpm_target=clip['bpm_int']))
    return store


def used_of(clip):
    from style.data import get_used_instruments
    return get_used_instruments(clip['instruments_features'], clip['unpitched'])


def batches(K):
    """Three different batches of K windows (every song and several first bars among them)."""
    from style.data import WindowBatch
    rng = np.random.default_rng(K)
    out = []
    for _ in range(3):
        ids = rng.integers(0, len(SONG_BARS), K)
        r0s = [int(rng.integers(0, SONG_BARS[s] - BARS + 1)) for s in ids]
        out.append(WindowBatch(C, BARS, T, True, ids, r0s))
    assert len({(tuple(b.songs), tuple(b.r0s)) for b in out}) == 3
    return out


def cropped(batch):
    """The batch's clips cropped on the host: [(pitched (1, C, BARS, T, 10, 56, 5), unpitched (1, 1, BARS, T, 10, 47, 2))]."""
    return [(songs()[s]['pitched'][:, :, r0:r0 + BARS].contiguous(), songs()[s]['unpitched'][:, :, r0:r0 + BARS].contiguous())
            for s, r0 in zip(batch.songs.tolist(), batch.r0s.tolist())]


def plan_reference(model, batch, clips_per_plan):
    """Gradient and K x 15 losses of the batch from plans driven directly: one Plan(clips=K) pass (clips_per_plan = K), or K
    passes of a one-clip plan on the tiling the batched plan chose, gradients accumulating (clips_per_plan = 1) — the two
    sides of parity_cases.batch_case."""
    from style import _native as nat
    native = nat.get()
    K = batch.K
    planK = nat.Plan(native, make_dims(pc.SMALL, C, BARS, T, True, clips=K), DEV)
    params = model._flat
    grads = torch.zeros_like(params)
    losses = torch.zeros(K, nat.N_LOSSES, device=DEV)
    dense = cropped(batch)
    inputs = lambda s: dict(mode=songs()[s]['mode'], bpm=songs()[s]['bpm'], instr=songs()[s]['instruments_features'],
                            used=used_of(songs()[s]), bpm_target=float(songs()[s]['bpm_int']))
    if clips_per_plan == K:
        for k, s in enumerate(batch.songs.tolist()):
            planK.set_inputs(clip=k, **inputs(s))
        xp, xu = torch.cat([p for p, _ in dense]).to(DEV), torch.cat([u for _, u in dense]).to(DEV)
        pc.poison(planK)
        planK.train_iteration(params, grads, xp, xu, losses)
    else:
        plan1 = nat.Plan(native, make_dims(pc.SMALL, C, BARS, T, True), DEV, gemm_tile=planK.gemm_tile)
        for k, s in enumerate(batch.songs.tolist()):
            plan1.set_inputs(**inputs(s))
            pc.poison(plan1)
            plan1.train_iteration(params, grads, dense[k][0].to(DEV), dense[k][1].to(DEV), losses[k])
    torch.cuda.synchronize()
    return grads.cpu(), losses.cpu(), planK.gemm_tile


@pytest.mark.parametrize('K,tile', [(3, 32), (8, 64)])
def test_train_windows_equals_the_batched_plan_on_host_cropped_clips(K, tile):
    """Three consecutive calls with different windows of one shape: eager, capture + replay, replay — each bit-identical, in
    gradients and per-clip losses, to Plan(clips=K).train_iteration on the host-cropped dense clips (same plan, same input
    bits), and within 2e-6 rel-L2 of K accumulating one-clip passes.  2e-6 is parity_cases.batch_case's bound for this very
    comparison, made as batch_case makes it: the one-clip plan on the tiling the batched plan chose (the sums differ in
    association only).  At K = 3 the model's own train_iteration is on that tiling by default and is compared as well."""
    model = build_model(pc.SMALL, seed=7).to(DEV)
    model._sync_flat()
    store = make_store()
    todo = batches(K)
    plan = model._plan(C, BARS, T, True, torch.device(DEV), clips=K)
    plan.__dict__.pop('_window_state', None)                            # (plans are cached per shape: start from a first use)
    for n, batch in enumerate(todo + todo[:1]):
        want_g, want_l, got_tile = plan_reference(model, batch, K)
        assert got_tile == tile
        model._gflat.zero_()
        got_l = model.train_windows(store, batch)
        torch.cuda.synchronize()
        assert got_l.shape == (K, 15) and torch.isfinite(got_l).all() and float(want_g.abs().sum()) > 0
        assert torch.equal(_bits(got_l.cpu()), _bits(want_l)), n
        assert torch.equal(_bits(model._gflat.cpu()), _bits(want_g)), n
        seq_g, seq_l, _ = plan_reference(model, batch, 1)
        e = rel(model._gflat.cpu().numpy(), seq_g.numpy())
        print(f'K={K} call {n}: rel-L2 to {K} one-clip passes {e:.3e}')
        assert e < 2e-6, (n, e)
        assert torch.equal(_bits(got_l.cpu()), _bits(seq_l)), n          # per-clip losses: bit-identical, as in batch_case
        assert (plan.__dict__['_window_state']['graph'] is not None) == (n >= 1)                 # a replay from the second use of the plan on
    if K == 3:
        grads = model._gflat.cpu().clone()                              # of todo[0], from a replay
        model._gflat.zero_()
        for (xp, xu), s in zip(cropped(todo[0]), todo[0].songs.tolist()):
            clip = songs()[s]
            model.train_iteration(clip['mode'].to(DEV), clip['bpm'].to(DEV), xp.to(DEV), clip['instruments_features'].to(DEV),
                                  xu.to(DEV), used_of(clip).to(DEV), clip['bpm_int'])
        torch.cuda.synchronize()
        e = rel(grads.numpy(), model._gflat.cpu().numpy())
        print(f'K=3: rel-L2 to 3 train_iteration calls {e:.3e}')
        assert e < 2e-6, e
    model.check_device_status()


def test_train_windows_leaves_the_lanes_alone():
    """Between the two train_iteration calls of an accumulation pair: the second call still takes lane 1 and gives the
    same losses and the same lane-1 gradient as without the batched pass in between."""
    from style.optim import FusedAdam
    store = make_store()
    batch = batches(3)[0]
    a, b = songs()[2], songs()[3]
    feed = lambda clip: (clip['mode'].to(DEV), clip['bpm'].to(DEV), clip['pitched'].to(DEV), clip['instruments_features'].to(DEV),
                         clip['unpitched'].to(DEV), used_of(clip).to(DEV), clip['bpm_int'])
    got = {}
    for interleave in (False, True):
        model = build_model(pc.SMALL, seed=7).to(DEV)
        opt = FusedAdam(model)                            # switches the two accumulation lanes on
        opt.zero_grad()
        model.train_iteration(*feed(a))
        if interleave:
            lane1 = model._lane_list[1]['grad']
            before = (model._lane_next, lane1.clone(), model._lane_list[1]['dirty'])
            losses = model.train_windows(store, batch)
            assert (model._lane_next, model._lane_list[1]['dirty']) == (before[0], before[2]) and model._lane_next == 1
            assert model._lane_list[1]['grad'] is lane1 and torch.equal(_bits(lane1), _bits(before[1]))
            assert torch.isfinite(losses).all()
        row = model.train_iteration(*feed(b))
        model.join_lanes_keep()
        torch.cuda.synchronize()
        got[interleave] = (row.cpu().clone(), model._lane_list[1]['grad'].cpu().clone(), model._gflat.cpu().clone())
        opt.zero_grad()
    assert torch.equal(_bits(got[True][0]), _bits(got[False][0])) and torch.isfinite(got[True][0][0])
    assert torch.equal(_bits(got[True][1]), _bits(got[False][1])) and float(got[True][1].abs().sum()) > 0
    assert not torch.equal(got[True][2], got[False][2])                 # the batch's gradient went into the model's buffer


# ---- the driver
def _driver_songs():
    """Small synthetic songs in get_input's form (float64 rolls); song 1 has no pitched notes and is skipped."""
    out = []
    for k, R in enumerate((3, 4, 4, 3, 5, 3)):
        clip = synth_clip(340 + k, 2, R, 4, True, density=.03)
        pitched, unpitched = clip['pitched'][0].double().numpy(), clip['unpitched'][0].double().numpy()
        if k == 1:
            pitched[:] = 0.
        info = dict(bpm=90 + 7 * k, scale=dict(mode='major' if k % 2 else 'minor'))
        out.append((f'song{k}', (info, pitched, clip['instruments_features'][0].double().numpy(), list(range(2)), unpitched)))
    return out


def test_train_with_windowed_batches(tmp_path):
    from style.train import build_model as build_full, train
    runs = []
    for n in range(2):
        path = str(tmp_path / f'training_{n}.csv')
        model = build_full(seed=108)
        start = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().clone()
        inputs = iter(_driver_songs())
        with pytest.warns(UserWarning, match='iter_size'):
            train(model, inputs, n_iterations=3, batch_clips=3, window_bars=2, store_songs=4, training_info_path=path, save_path=None,
                  progress=False)
        assert [s[0] for s in inputs] == ['song5']                       # songs 0, 2, 3, 4 went into the store; song 1 was skipped
        rows = list(csv.reader(open(path)))
        assert len(rows) == 1 + 3 and [r[0] for r in rows[1:]] == ['0', '1', '2']
        assert all(np.isfinite(float(r[1])) for r in rows[1:]) and all(r[8] != '' for r in rows[1:])
        end = model._flat.detach().cpu().clone()
        assert torch.isfinite(end).all() and not torch.equal(end, start)
        runs.append((rows, end))
    assert runs[0][0] == runs[1][0] and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
