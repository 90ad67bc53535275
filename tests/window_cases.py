"""mst_clip_window cases shared by the CPU-interpreter tests and the -m gpu tests: both drive the SAME C ABI; only the library
build (hipsim vs hipcc/gfx950) and the device differ.  Every comparison is bit equality against `x[:, :, r0:r0 + bars]` of the
dense song, zero-extended in numpy, into a NaN-poisoned destination."""
import numpy as np
import torch

from tools.synth import synth_clip

NAN = float('nan')
SONGS = ((2, 3, 1), (2, 5, 1), (2, 2, 1))        # (C, R_song, T) of the pool's three songs: `first` is non-zero for two of them
_cache = {}


def songs():
    """The three songs' dense rolls, computed once: [(pitched (C, R, 560 T, 5), unpitched (1, R, 470 T, 2))] as numpy."""
    if 'songs' not in _cache:
        out = []
        for k, (C, R, T) in enumerate(SONGS):
            clip = synth_clip(70 + k, C, R, T, True, density=.05)
            out.append((clip['pitched'].numpy().reshape(C, R, T * 560, 5), clip['unpitched'].numpy().reshape(1, R, T * 470, 2)))
        _cache['songs'] = out
    return _cache['songs']


def records(x):
    """(cells int32, feats float32) of a dense roll (channels, bars, bar_cells, nfeat): the cells with a non-zero bit pattern."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).reshape(-1, x.shape[-1])
    cells = np.flatnonzero(bits.any(axis=1))
    return cells.astype(np.int32), np.ascontiguousarray(x, dtype=np.float32).reshape(bits.shape)[cells]


class Pool:
    """Records of several rolls back to back, on `device`, and where each roll's records start."""

    def __init__(self, rolls, device):
        recs = [r if isinstance(r, tuple) else records(r) for r in rolls]
        self.first = np.cumsum([0] + [len(c) for c, _ in recs])[:-1].tolist()
        self.count = [len(c) for c, _ in recs]
        self.cells = torch.from_numpy(np.concatenate([c for c, _ in recs])).to(device)
        self.feats = torch.from_numpy(np.concatenate([f for _, f in recs])).to(device)


def reference(x, r0, bars):
    """x[:, r0:r0 + bars] of the dense roll, zero-extended on both sides."""
    out = np.zeros((x.shape[0], bars) + x.shape[2:], dtype=np.float32)
    for r in range(bars):
        if 0 <= r0 + r < x.shape[1]:
            out[:, r] = x[:, r0 + r]
    return out


def crop(native, device, pool, rolls, clips, bars, lead=0, counts=None, src_bars=None):
    """Run mst_clip_window for `clips` = [(roll index, r0)] into a NaN-poisoned buffer, `lead` floats into it; checks that the
    NaNs around the destination are untouched and returns the destination as numpy (K, channels, bars, bar_cells, nfeat)."""
    channels, _, bar_cells, nfeat = rolls[0].shape
    win = np.array([[pool.first[i], pool.count[i] if counts is None else counts[k],
                     rolls[i].shape[1] if src_bars is None else src_bars[k], r0] for k, (i, r0) in enumerate(clips)], dtype=np.int32)
    n = len(clips) * channels * bars * bar_cells * nfeat
    buf = torch.full((n + 8,), NAN, device=device)
    native.clip_window(pool.cells, pool.feats, torch.from_numpy(win).to(device), buf[lead:lead + n], len(clips), channels, bars,
                       bar_cells, nfeat, stream=None if torch.device(device).type == 'cpu' else torch.cuda.current_stream(device).cuda_stream)
    host = buf.cpu()
    assert torch.isnan(host[:lead]).all() and torch.isnan(host[lead + n:]).all(), 'floats outside the destination were written'
    return host[lead:lead + n].numpy().reshape(len(clips), channels, bars, bar_cells, nfeat)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def check(native, device, rolls, clips, bars, pool=None, **kw):
    pool = pool or Pool(rolls, device)
    got = crop(native, device, pool, rolls, clips, bars, **kw)
    want = np.stack([reference(rolls[i], r0, bars) for i, r0 in clips])
    assert not np.isnan(got).any(), 'a float of the destination was not written'
    assert same_bits(got, want), [k for k in range(len(clips)) if not same_bits(got[k], want[k])]
    return got


def both(which):
    return [s[which] for s in songs()]


# ---- the cases
def case_one_clip_per_song(native, device):
    """bars = 2, three clips, one per song: r0 at the start, in the middle and at R_song - bars."""
    for which in (0, 1):
        rolls = both(which)
        check(native, device, rolls, [(0, 0), (1, 2), (2, 0)], 2)
        check(native, device, rolls, [(0, 1), (1, 3), (1, 1)], 2)


def case_slices_span_slabs_and_clips(native, device):
    """bars = 1 on the unpitched rolls: a slab is 940 floats, so a 2048-float slice spans slabs and clips."""
    rolls = both(1)
    clips = [(i, r0) for i, (_, R, _) in enumerate(SONGS) for r0 in range(R)]
    assert rolls[0].shape[2] * 2 == 940 and len(clips) == 10
    got = check(native, device, rolls, clips, 1)
    assert (got != 0).any()
    check(native, device, both(0), clips, 1)               # and the pitched rolls: two channels, two slabs per clip


def case_windows_outside_the_song(native, device):
    """r0 = -1 and r0 = R_song - 1 are partly outside, r0 = -bars, R_song and far away wholly: zeros where there is no song."""
    for which in (0, 1):
        rolls = both(which)
        R = [r.shape[1] for r in rolls]
        got = check(native, device, rolls, [(0, -1), (1, R[1] - 1), (2, -1), (2, R[2] - 1)], 2)
        assert (got[0, :, 0] == 0).all() and (got[0, :, 1] != 0).any() and (got[1, :, 1] == 0).all() and (got[1, :, 0] != 0).any()
        got = check(native, device, rolls, [(0, -2), (1, R[1]), (2, 2 ** 31 - 1), (0, -2 ** 31), (1, 1)], 2)
        assert (got[:4] == 0).all() and (got[4] != 0).any()


def case_unaligned_destinations(native, device):
    """Destinations 1, 2 and 3 floats off a 16-byte boundary: same bits, and the NaNs around them stay (crop checks)."""
    for which in (0, 1):
        rolls = both(which)
        pool = Pool(rolls, device)
        for lead in (1, 2, 3):
            check(native, device, rolls, [(1, 1), (0, 2), (2, 0)], 2, pool=pool, lead=lead)


def big_song():
    if 'big' not in _cache:
        clip = synth_clip(6, 1, 35, 4, True, density=1.)       # as tests/test_sparse_clip.py: more than 65536 records per roll
        _cache['big'] = (clip['pitched'].numpy().reshape(1, 35, 4 * 560, 5), clip['unpitched'].numpy().reshape(1, 35, 4 * 470, 2))
    return _cache['big']


def case_more_than_64k_records(native, device):
    """One song of more than 65536 records cropped to 2 bars: the workgroup-wide search takes its third round."""
    for which in (0, 1):
        small, x = songs()[0][which], big_song()[which]
        if small.shape[0] != 1:
            small = small[:1]
        rolls = [np.ascontiguousarray(np.repeat(small, 4, axis=2)), x]      # a small song in front: `first` is non-zero
        assert rolls[0].shape[2:] == x.shape[2:]
        pool = Pool(rolls, device)
        assert pool.count[1] > 1 << 16 and pool.first[1] > 0
        check(native, device, rolls, [(1, 17), (1, 0), (1, 33), (1, 34)], 2, pool=pool)


def case_negative_count(native, device):
    """A negative count is clamped at 0: the clip comes out as zeros, its neighbours as they are."""
    rolls = both(1)
    pool = Pool(rolls, device)
    got = crop(native, device, pool, rolls, [(0, 0), (1, 1), (2, 0)], 2, counts=[pool.count[0], -5, pool.count[2]])
    assert same_bits(got[0], reference(rolls[0], 0, 2)) and same_bits(got[2], reference(rolls[2], 0, 2))
    assert same_bits(got[1], np.zeros_like(got[1]))


def case_cell_beyond_the_roll(native, device):
    """One record whose cell lies beyond its song's roll is skipped, never stored: the window that reaches past the end of
    the song would otherwise show it in the bar after the last."""
    for which in (0, 1):
        rolls = both(which)
        recs = [records(r) for r in rolls]
        channels, R, bar_cells, nfeat = rolls[1].shape
        cells, feats = recs[1]
        beyond = channels * R * bar_cells + 3                  # bar R of the last channel, were there one
        recs[1] = (np.append(cells, np.int32(beyond)), np.concatenate([feats, np.full((1, nfeat), 7., np.float32)]))
        pool = Pool(recs, device)
        assert pool.count[1] == len(cells) + 1
        check(native, device, rolls, [(0, 0), (1, R - 1), (1, R - 2), (2, 0)], 2, pool=pool)


def case_err_arg(native, device):
    """Every MST_ERR_ARG case; nothing is written by a refused call."""
    rolls = both(1)
    pool = Pool(rolls, device)
    win = torch.tensor([[0, pool.count[0], 3, 0]], dtype=torch.int32, device=device)
    out = torch.full((2 * 470 * 2,), NAN, device=device)
    P = lambda t: t.data_ptr()
    call = native.lib.mst_clip_window
    good = (P(pool.cells), P(pool.feats), P(win), 1, 1, 2, 470, 2, P(out), None)
    assert call(*good) == 0
    after = out.cpu().clone()
    assert not torch.isnan(after).any()
    out.fill_(NAN)

    def but(**kw):
        names = ('cells', 'feats', 'win', 'n_clips', 'channels', 'bars', 'bar_cells', 'nfeat', 'out', 'stream')
        args = dict(zip(names, good))
        args.update(kw)
        return tuple(args[n] for n in names)
    bad = [but(cells=None), but(feats=None), but(win=None), but(out=None), but(nfeat=3), but(nfeat=0), but(nfeat=4), but(n_clips=0),
           but(n_clips=-1), but(channels=0), but(bars=0), but(bars=-2), but(bar_cells=0), but(bar_cells=-470),
           but(bar_cells=2 ** 31), but(bars=2 ** 20, bar_cells=2 ** 11), but(channels=2 ** 10, bars=2 ** 10, bar_cells=2 ** 11)]
    for args in bad:
        assert call(*args) == -1, args                     # MST_ERR_ARG
    assert torch.isnan(out.cpu()).all()


def case_two_runs_are_bit_identical(native, device):
    for which in (0, 1):
        rolls = both(which)
        pool = Pool(rolls, device)
        clips = [(1, 2), (0, -1), (2, 1), (1, 0)]
        a = crop(native, device, pool, rolls, clips, 2)
        b = crop(native, device, pool, rolls, clips, 2, lead=0)
        assert same_bits(a, b)


CASES = [case_one_clip_per_song, case_slices_span_slabs_and_clips, case_windows_outside_the_song, case_unaligned_destinations,
         case_more_than_64k_records, case_negative_count, case_cell_beyond_the_roll, case_err_arg, case_two_runs_are_bit_identical]
