"""Windowed clips on the CPU: mst_clip_window (the product's kernel source on the hipsim interpreter, the cases of
tests/window_cases.py) and the host side of style.data.SongStore — buckets, reproducible sampling, the silence rule."""
import numpy as np
import pytest
import torch

import simutil
import window_cases as wc
from tools.synth import synth_clip


@pytest.mark.parametrize('case', wc.CASES, ids=[c.__name__[5:] for c in wc.CASES])
def test_clip_window(case):
    case(simutil.sim_native(), 'cpu')


# ---- SongStore, host only
def _clip(k, C, R, T, percussion=True, density=.05, drums_in_bar=None):
    from style.data import SparseClip, sparsify
    clip = synth_clip(200 + k, C, R, T, True, density=density)
    unpitched = clip['unpitched']
    if drums_in_bar is not None:
        keep = unpitched[:, :, drums_in_bar].clone()
        unpitched = torch.zeros_like(unpitched)
        unpitched[:, :, drums_in_bar] = keep
    return SparseClip(clip['mode'], clip['bpm'], sparsify(clip['pitched'], pin=False), clip['instruments_features'],
                      sparsify(unpitched, pin=False) if percussion else None, bpm_target=90 + k, pin=False)


def _store(specs):
    from style.data import SongStore
    store = SongStore('cpu', capacity=64)              # a small pool: it has to grow by doubling on the way
    ids = [store.add(_clip(k, *spec)) for k, spec in enumerate(specs)]
    assert ids == list(range(len(specs))) and len(store) == len(specs)
    return store


SPECS = [(2, 5, 1), (2, 3, 1), (1, 4, 1), (2, 6, 1, False), (2, 4, 2), (2, 7, 1)]


def test_bucket_keys_pools_and_table():
    store = _store(SPECS)
    assert set(store.buckets) == {(2, 1, True), (1, 1, True), (2, 1, False), (2, 2, True)}
    assert store.buckets[(2, 1, True)]['songs'] == [0, 1, 5] and store.buckets[(2, 1, False)]['songs'] == [3]
    assert [store.bucket_of(s) for s in range(6)] == [(2, 1, True), (2, 1, True), (1, 1, True), (2, 1, False), (2, 2, True), (2, 1, True)]
    # a clip whose percussion is silent goes in without it, as drop_silent would have it; one without pitched notes is refused
    silent_drums = _clip(9, 2, 3, 1, density=.05)
    silent_drums.unpitched_channels.feats.zero_()
    assert store.bucket_of(store.add(silent_drums)) == (2, 1, False)
    nothing = _clip(10, 2, 3, 1)
    nothing.pitched_channels.feats.zero_()
    with pytest.raises(ValueError):
        store.add(nothing)
    # the pools hold every song's records back to back, the table its small inputs
    at = {5: 0, 2: 0}
    for k, spec in enumerate(SPECS):
        clip, song = _clip(k, *spec), store.songs[k]
        for nfeat, name, roll in ((5, 'pitched', clip.pitched_channels), (2, 'unpitched', clip.unpitched_channels)):
            if roll is None:
                assert song[name] is None
                continue
            first, count = song[name]
            assert (first, count) == (at[nfeat], roll.count)
            at[nfeat] += count
            assert torch.equal(store.pools[nfeat].cells[first:first + count], roll.cells)
            assert torch.equal(store.pools[nfeat].feats[first:first + count], roll.feats)
        from style.data import WindowBatch, get_used_instruments
        views = store.small_inputs(WindowBatch(spec[0], 1, spec[2], song['percussion'], [k], [0]))
        want = (clip.mode, clip.bpm, clip.instruments_features, get_used_instruments(clip.instruments_features, clip.unpitched_channels),
                torch.tensor([float(clip.bpm_target)]))
        assert len(views) == 5 and all(torch.equal(v, w.reshape(-1)) for v, w in zip(views, want))
    assert store.pools[5].cells.numel() > 64 and store.pools[5].used == at[5] + silent_drums.pitched_channels.count
    assert store.pools[2].used == at[2]                    # the silent percussion was not stored


def test_sample_is_reproducible_and_uniform_in_shape():
    store = _store(SPECS)
    draws = [[store.sample(np.random.default_rng(seed), 5, 2) for _ in range(2)] for seed in (3, 3, 4)]
    for a, b in zip(draws[0], draws[1]):
        assert (a.C, a.bars, a.T, a.percussion) == (b.C, b.bars, b.T, b.percussion)
        assert np.array_equal(a.songs, b.songs) and np.array_equal(a.r0s, b.r0s)
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(40):
        batch = store.sample(rng, 4, 3)
        key = (batch.C, batch.T, batch.percussion)
        seen.add(key)
        assert batch.K == 4 and batch.bars == 3
        for song, r0 in zip(batch.songs, batch.r0s):
            assert store.bucket_of(song) == key and 0 <= r0 <= store.songs[song]['R'] - 3
    assert len(seen) == 4                                  # every bucket has a song of 3 bars or more
    out = np.zeros((2, 4, 4), np.int32)
    store.describe(batch, out)
    for k, (song, r0) in enumerate(zip(batch.songs, batch.r0s)):
        assert tuple(out[0, k]) == (*store.songs[song]['pitched'], store.songs[song]['R'], r0)


def _dense_window(clip, r0, bars):
    p = clip.pitched_channels.to_numpy()[0, :, r0:r0 + bars]
    u = None if clip.unpitched_channels is None else clip.unpitched_channels.to_numpy()[0, :, r0:r0 + bars]
    return p, u


def test_every_window_passes_the_silence_rule():
    """One song's percussion sits in bar 9 of 12 only: of its 11 two-bar windows 2 may be drawn."""
    from style.data import SongStore
    store = SongStore('cpu')
    clips = [_clip(0, 2, 12, 1, drums_in_bar=9), _clip(1, 2, 4, 1, density=.002)]
    for clip in clips:
        store.add(clip)
    rng = np.random.default_rng(11)
    r0s = {0: set(), 1: set()}
    for _ in range(30):
        batch = store.sample(rng, 6, 2)
        for song, r0 in zip(batch.songs.tolist(), batch.r0s.tolist()):
            p, u = _dense_window(clips[song], r0, 2)
            assert np.any(p) and np.any(u), (song, r0)
            assert store.window_sounds(song, r0, 2)
            r0s[song].add(r0)
    assert r0s[0] == {8, 9}
    # window_sounds is the dense rule for every window of both songs
    for song, clip in enumerate(clips):
        for r0 in range(store.songs[song]['R'] - 1):
            p, u = _dense_window(clip, r0, 2)
            assert store.window_sounds(song, r0, 2) == bool(np.any(p) and np.any(u)), (song, r0)


def test_none_when_no_bucket_can_fill_the_slots():
    from style.data import SongStore
    store = _store(SPECS)
    assert store.sample(np.random.default_rng(0), 3, 8) is None           # longer than every song
    assert store.sample(np.random.default_rng(0), 3, 7).songs.tolist() == [5, 5, 5]
    only_silent = SongStore('cpu')
    clip = _clip(3, 1, 6, 1, drums_in_bar=0)
    clip.pitched_channels.feats.numpy()[clip.pitched_channels.cells.numpy() < 3 * 560] = 0.     # pitched notes in bars 3-5 only
    only_silent.add(clip)
    assert only_silent.sample(np.random.default_rng(0), 2, 2) is None      # no window has both
    assert only_silent.sample(np.random.default_rng(0), 2, 4).r0s.tolist() == [0, 0]


def test_sampled_windows_through_the_kernel():
    """store.sample -> store.describe -> mst_clip_window over the store's pools gives the windows of the dense songs."""
    store = _store(SPECS)
    clips = [_clip(k, *spec) for k, spec in enumerate(SPECS)]
    rng = np.random.default_rng(2)
    native = simutil.sim_native()
    seen = set()
    for _ in range(8):
        batch = store.sample(rng, 5, 2)
        seen.add(batch.percussion)
        win = torch.zeros(2, batch.K, 4, dtype=torch.int32)
        store.describe(batch, win.numpy())
        pitched = torch.full((batch.K, batch.C, 2, batch.T, 10, 56, 5), float('nan'))
        native.clip_window(store.pools[5].cells, store.pools[5].feats, win[0], pitched, batch.K, batch.C, 2, batch.T * 560, 5)
        unpitched = torch.full((batch.K, 1, 2, batch.T, 10, 47, 2), float('nan'))
        if batch.percussion:
            native.clip_window(store.pools[2].cells, store.pools[2].feats, win[1], unpitched, batch.K, 1, 2, batch.T * 470, 2)
        else:
            assert not win[1].any()
        for k, (song, r0) in enumerate(zip(batch.songs.tolist(), batch.r0s.tolist())):
            p, u = _dense_window(clips[song], r0, 2)
            assert wc.same_bits(pitched[k].numpy(), p)
            assert u is None or wc.same_bits(unpitched[k].numpy(), u)
    assert seen == {True, False}
