"""-m gpu: the rotating song store on an MI355X.  mst_store_admit (the cases of tests/admit_cases.py on the gfx950 build), the
scripted admit sequence through the kernel with every window cropped by mst_clip_window, train_windows / eval_windows on a ring
store against an append-only store holding the same songs — before and after an admit that wraps and evicts, on ONE captured
graph — and style.train.train(refresh_every=...)."""
import csv

import numpy as np
import pytest
import torch

import admit_cases as ac
import parity_cases as pc
from test_host_surface import build_model
from tools.synth import synth_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C, T, BARS, K = 2, 2, 2, 3
SONG_BARS = (2, 5, 3, 4, 3, 4)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize('case', ac.CASES + [ac.case_ring_crops_equal_the_append_only_store],
                         ids=[c.__name__[5:] for c in ac.CASES] + ['script_through_the_kernel'])
def test_store_admit(case):
    from style import _native
    case(_native.get(), DEV)
    torch.cuda.synchronize()


# ---- train_windows / eval_windows on a ring store
_songs = []


def songs():
    """Six songs of 2 to 5 bars (C = 2, T = 2, with percussion) as SparseClips, each with its own mode, bpm and instruments."""
    from style.data import SparseClip, sparsify
    if not _songs:
        for k, R in enumerate(SONG_BARS):
            clip = synth_clip(700 + k, C, R, T, True, density=.05, bpm=80 + 11 * k)
            mode = torch.tensor([[0., 1.]]) if k % 2 else clip['mode']
            feats = torch.zeros_like(clip['instruments_features'])
            for c in range(C):
                feats[0, c, (3 * k + c) % 40] = 1.
                feats[0, c, 40 + (k + c) % 11] = 1.
            _songs.append(SparseClip(mode, clip['bpm'], sparsify(clip['pitched'], pin=False), feats, sparsify(clip['unpitched'], pin=False),
                                     bpm_target=clip['bpm_int'], pin=False))
    return _songs


def ring_of_four():
    """A ring that holds songs 0-3 with a few records to spare: song 4 wraps to record 0 and evicts songs 0 and 1."""
    from style.data import SongStore
    capacity = sum(-(-s.pitched_channels.count // 4) * 4 for s in songs()[:4]) + 8
    store = SongStore(DEV, capacity=capacity, resident=4)
    assert store.admit(songs()[:4]) == [0, 1, 2, 3]
    return store


def twin_of(store):
    """An append-only store holding the ring's resident songs, and the ring id -> twin id map."""
    from style.data import SongStore
    twin = SongStore(DEV, capacity=256)
    return twin, {i: twin.add(songs()[i]) for i in store.resident()}


def batches_of(store, seed):
    """Three different batches of K windows of the ring's resident songs."""
    from style.data import WindowBatch
    rng = np.random.default_rng(seed)
    live = store.resident()
    out = []
    for _ in range(3):
        ids = [live[int(i)] for i in rng.integers(0, len(live), K)]
        out.append(WindowBatch(C, BARS, T, True, ids, [int(rng.integers(0, SONG_BARS[s] - BARS + 1)) for s in ids]))
    return out


def mapped(batch, ids):
    from style.data import WindowBatch
    return WindowBatch(batch.C, batch.bars, batch.T, batch.percussion, [ids[int(s)] for s in batch.songs], batch.r0s)


def small_model():
    model = build_model(pc.SMALL, seed=7).to(DEV)
    model._sync_flat()
    return model


def _train_windows(model, store, batch):
    model._gflat.zero_()
    losses = model.train_windows(store, batch)
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and float(model._gflat.abs().sum()) > 0
    return _bits(losses).clone(), _bits(model._gflat).clone()


def test_train_windows_on_a_ring_store_across_a_refresh():
    """Losses and the gradient buffer are bit-identical to train_windows on an append-only store with the same songs, before
    and after an admit that wraps and evicts; the plan's captured graph is the SAME object after the admit, and no pool moved."""
    from style.data import SongEvicted
    model = small_model()
    plan = model._plan(C, BARS, T, True, torch.device(DEV), clips=K)
    plan.__dict__.pop('_window_state', None)                            # (plans are cached per shape: start from a first use)
    ring = ring_of_four()
    ptrs = [t.data_ptr() for p in ring.pools.values() for t in (p.cells, p.feats)]
    before = batches_of(ring, 1)
    got = [_train_windows(model, ring, b) for b in before]              # eager, capture + replay, replay
    graph = plan.__dict__['_window_state']['graph']
    assert graph is not None
    twin_before = twin_of(ring)
    assert ring.admit(songs()[4:5]) == [4]
    assert ring.resident() == [2, 3, 4] and ring.songs[4]['pitched'][0] == 0 and ring.evicted(0) and ring.evicted(1)
    after = batches_of(ring, 2)
    assert any(4 in b.songs for b in after)
    got += [_train_windows(model, ring, b) for b in after]
    ring.check()
    assert plan.__dict__['_window_state']['graph'] is graph, 'the admit made train_windows capture again'
    assert ptrs == [t.data_ptr() for p in ring.pools.values() for t in (p.cells, p.feats)]
    stale = [b for b in before if set(b.songs.tolist()) & {0, 1}]
    assert stale
    with pytest.raises(SongEvicted):
        model.train_windows(ring, stale[0])
    # the same batches on append-only stores holding the same songs
    twin_after = twin_of(ring)
    want = [_train_windows(model, twin_before[0], mapped(b, twin_before[1])) for b in before]
    want += [_train_windows(model, twin_after[0], mapped(b, twin_after[1])) for b in after]
    for n, ((gl, gg), (wl, wg)) in enumerate(zip(got, want)):
        assert torch.equal(gl, wl) and torch.equal(gg, wg), n
    model.check_device_status()


def test_eval_windows_on_a_ring_store_after_a_refresh():
    """The 41 doubles of a round (and the per-clip losses and metrics) equal those of the append-only twin, bit for bit."""
    model = small_model()
    ring = ring_of_four()
    ring.admit(songs()[4:6])
    ring.check()
    assert 5 in ring.resident() and ring.evicted(0)
    twin, ids = twin_of(ring)
    acc = model.eval_accumulator()
    results = []
    for store, rename in ((ring, None), (twin, ids), (ring, None)):
        acc.zero_()
        parts = []
        for n, batch in enumerate(batches_of(ring, 3)):
            losses, metrics = model.eval_windows(store, batch if rename is None else mapped(batch, rename), live=K - (n == 2), acc=acc)
            parts += [_bits(losses).clone(), metrics.detach().cpu().view(torch.int64).clone()]
        torch.cuda.synchronize()
        results.append((acc.cpu().view(torch.int64).clone(), parts))
    assert float(results[0][0].view(torch.float64).abs().sum()) > 0
    for other in results[1:]:
        assert torch.equal(results[0][0], other[0])
        assert all(torch.equal(a, b) for a, b in zip(results[0][1], other[1]))
    model.check_device_status()


# ---- the driver
def driver_songs(n=10):
    """Small synthetic songs in get_input's form (float64 rolls); song 1 has no pitched notes and is skipped."""
    out = []
    for k in range(n):
        clip = synth_clip(740 + k, C, (3, 4, 2, 3, 5, 3, 4, 2, 3, 4)[k % 10], T, True, density=.04)
        pitched, unpitched = clip['pitched'][0].double().numpy(), clip['unpitched'][0].double().numpy()
        if k == 1:
            pitched[:] = 0.
        info = dict(bpm=90 + 7 * k, scale=dict(mode='major' if k % 2 else 'minor'))
        out.append((f'song{k}', (info, pitched, clip['instruments_features'][0].double().numpy(), list(range(C)), unpitched)))
    return out


def run_train(tmp_path, name, n_songs=10, n_iterations=6, **kw):
    from style.train import train
    model = build_model(pc.SMALL, seed=7).to(DEV)
    path = str(tmp_path / f'{name}.csv')
    with pytest.warns(UserWarning, match='iter_size'):
        train(model, iter(driver_songs(n_songs)), n_iterations=n_iterations, batch_clips=K, window_bars=BARS, store_songs=3,
              training_info_path=path, save_path=None, progress=False, **kw)
    torch.cuda.synchronize()
    rows = list(csv.reader(open(path)))[1:]
    assert [r[0] for r in rows] == [str(i) for i in range(n_iterations)] and all(np.isfinite(float(r[1])) for r in rows)
    return rows, _bits(model._flat).clone()


def test_train_with_a_rotating_store(tmp_path):
    from style.data import SongStore
    from style.optim import FusedAdam
    from style.train import iter_sparse
    runs = [run_train(tmp_path, f'rotating{n}', refresh_every=2, refresh_songs=2) for n in range(2)]
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    # until the first refresh: the same store contents and the same rng stream as the loop without one
    plain = run_train(tmp_path, 'plain')
    assert plain[0][:2] == runs[0][0][:2] and all(a != b for a, b in zip(plain[0][2:], runs[0][0][2:]))
    assert not torch.equal(plain[1], runs[0][1])
    # the whole trajectory from the public pieces, in the stated order: this pins which songs are admitted when
    clips = [c for c in iter_sparse(iter(driver_songs())) if c is not None]
    total = max(sum(c.pitched_channels.count for c in clips[:3]), sum(c.unpitched_channels.count for c in clips[:3]))
    capacity = 1
    while capacity < 2 * total:
        capacity *= 2
    model = build_model(pc.SMALL, seed=7).to(DEV)
    opt = FusedAdam(model, lr=.01, step_size=200, gamma=.9)
    opt.zero_grad()
    store = SongStore(DEV, capacity=capacity, resident=3)
    store.admit(clips[:3])
    rng, at, rows = np.random.default_rng(0), 3, []
    for iteration in range(6):
        rows.append(model.train_windows(store, store.sample(rng, K, BARS)).mean(0))
        opt.step()
        if (iteration + 1) % 2 == 0:
            store.admit(clips[at:at + 2])
            at += 2
    store.check()
    assert store.resident() == [6, 7, 8] and len(store) == 9
    rows = torch.stack(rows).cpu().numpy()
    for mine, (_, *theirs) in zip(rows.tolist(), runs[0][0]):
        assert [x for x in mine if not np.isnan(x)] == [float(x) for x in theirs if x != '']
    assert torch.equal(_bits(model._flat), runs[0][1])


def test_inputs_that_run_out_end_the_run_normally(tmp_path):
    """Eight songs, seven usable: three fill the ring, two refreshes take two each, the third finds none; training goes on."""
    rows, _ = run_train(tmp_path, 'short', n_songs=8, n_iterations=8, refresh_every=2, refresh_songs=2)
    assert len(rows) == 8
