"""mst_store_admit and the ring mode of style.data.SongStore: cases shared by the CPU tests (the kernel on the hipsim interpreter,
the store on the host) and the -m gpu tests — both drive the SAME C ABI; only the library build and the device differ.  Kernel
cases copy into NaN-poisoned destinations with guard words on both sides and compare WHOLE buffers, as int32, with a host model
of the copy rule of include/mst_amd.h.  Store cases run a scripted admit sequence and check, after every step, the ring's
invariants against the source clips."""
import ctypes

import numpy as np
import torch

from tools.synth import synth_clip

GUARD = 8
POISON = 0x7fc0beef                      # a NaN with payload bits
LENGTHS = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)
# NaNs with payload bits (quiet, signalling, negative), 0x80000000 (-0.0 as a float, the smallest cell as an int), denormals
SPECIAL = np.array([0x7fc00001, 0x7f800123, 0xffc12345, 0x80000000, 0x00000001, 0x807fffff, 0x00000000, 0x3f800000], dtype=np.uint32).view(np.int32)
N_DSTS = 16


class Dst:
    """A destination of `words` words inside a poisoned buffer, GUARD words on both sides, `lead` words off the buffer's start
    (lead = 1: a base pointer that is 4-byte aligned only)."""

    def __init__(self, words, device, lead=0):
        self.words, self.lead = words, lead
        self.buf = torch.full((lead + GUARD + words + GUARD,), POISON, dtype=torch.int32, device=device)

    @property
    def addr(self):
        return self.buf.data_ptr() + 4 * (self.lead + GUARD)

    def host(self):
        return self.buf.cpu().numpy()


def _stream(device):
    return None if torch.device(device).type == 'cpu' else torch.cuda.current_stream(device).cuda_stream


def payload(rng, n):
    """n words of every bit pattern, the special ones sprinkled in."""
    x = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    if n:
        at = rng.integers(0, n, max(1, n // 7))
        x[at] = SPECIAL[rng.integers(0, len(SPECIAL), len(at))]
    return x


def make_blob(segments, max_segments, words, seed=0, n=None):
    """Header of `segments` [(dst, dst_off, src_off, words)] and a payload of `words` words in all."""
    blob = np.zeros(words, dtype=np.int32)
    head = 4 + 4 * max_segments
    blob[head:] = payload(np.random.default_rng(seed), words - head)
    blob[0] = len(segments) if n is None else n
    blob[1:4] = (-1, 2 ** 31 - 1, 77)                          # never read
    for i, s in enumerate(segments):
        blob[4 + 4 * i:8 + 4 * i] = s
    return blob


def model(blob, max_segments, blob_words, dsts):
    """The copy rule on the host: the expected buffers (guards included) and status words."""
    images = [None if x is None else np.full(x.buf.numel(), POISON, np.int32) for x in dsts]
    status = np.zeros(max_segments, np.int32)
    n = min(max(int(blob[0]), 0), max_segments)
    for i in range(n):
        dst, dst_off, src_off, words = (int(v) for v in blob[4 + 4 * i:8 + 4 * i])
        ok = (0 <= dst < N_DSTS and dst < len(dsts) and dsts[dst] is not None and words >= 0 and src_off >= 4 + 4 * max_segments
              and src_off + words <= blob_words and dst_off >= 0 and dst_off + words <= dsts[dst].words)
        if not ok:
            status[i] = 1
            continue
        at = dsts[dst].lead + GUARD + dst_off
        images[dst][at:at + words] = blob[src_off:src_off + words]
    return images, status


def launch(native, device, blob, max_segments, dsts, blob_words=None, seed=5):
    """-> the status words, which were garbage before the launch."""
    from style import _native as nat
    table = nat.AdmitDsts()
    for k, x in enumerate(dsts):
        if x is not None:
            table.set(k, x.addr, x.words)
    garbage = np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, max_segments, dtype=np.int64).astype(np.int32)
    garbage[garbage == 0] = 9
    garbage[garbage == 1] = 9
    status = torch.from_numpy(garbage).to(device)
    native.store_admit(torch.from_numpy(blob).to(device), len(blob) if blob_words is None else blob_words, max_segments, table, status,
                       _stream(device))
    return status.cpu().numpy()


def check(native, device, blob, max_segments, dsts, blob_words=None):
    want, want_status = model(blob, max_segments, len(blob) if blob_words is None else blob_words, dsts)
    status = launch(native, device, blob, max_segments, dsts, blob_words)
    assert set(np.unique(status).tolist()) <= {0, 1}, 'a status word is neither 0 nor 1'
    assert np.array_equal(status, want_status), np.flatnonzero(status != want_status)[:8]
    for k, (x, image) in enumerate(zip(dsts, want)):
        if x is not None:
            got = x.host()
            assert np.array_equal(got, image), (k, np.flatnonzero(got != image)[:8])
    return status


# ---- the kernel's cases
def case_lengths_and_alignment(native, device):
    """Every length with every residue mod 4 of the source and of the destination offset — the 16-byte path with head and tail
    where they agree, the word path where they do not — into a 16-byte-aligned destination and into one a float off."""
    for lead in (0, 1):
        max_segments = len(LENGTHS) * 16
        segments, src, dst = [], 4 + 4 * max_segments, 0
        for length in LENGTHS:
            for rs in range(4):
                for rd in range(4):
                    src += (rs - src) % 4
                    dst += 1 + (rd - dst - 1) % 4             # at least one poisoned word between two destination ranges
                    assert src % 4 == rs and dst % 4 == rd
                    segments.append((0, dst, src, length))
                    src, dst = src + length, dst + length
        x = Dst(dst + 3, device, lead=lead)
        status = check(native, device, make_blob(segments, max_segments, src + 5, seed=lead), max_segments, [x])
        assert not status.any() and (x.host() != POISON).sum() > sum(LENGTHS) * 15


def case_more_segments_than_one_round(native, device):
    """n = max_segments = 300 short segments over three destinations: the header is read in more than one round of 256."""
    rng = np.random.default_rng(3)
    max_segments, segments, src, at = 300, [], 4 + 4 * 300, [0, 0, 0]
    for i in range(max_segments):
        length, d = int(rng.integers(0, 10)), i % 3
        segments.append((d, at[d], src, length))
        src, at[d] = src + length, at[d] + length + int(rng.integers(0, 3))
    dsts = [Dst(at[d] + 2, device, lead=d) for d in range(3)]
    assert not check(native, device, make_blob(segments, max_segments, src), max_segments, dsts).any()


def case_segment_counts(native, device):
    """n = 0 writes nothing; blob[0] above max_segments is clamped; a negative blob[0] behaves as 0."""
    max_segments = 4
    head = 4 + 4 * max_segments
    segments = [(0, 10 * i, head + 8 * i, 7) for i in range(max_segments)]
    for n, copied in ((0, 0), (max_segments, 4), (max_segments + 5, 4), (2 ** 31 - 1, 4), (-3, 0), (-2 ** 31, 0), (2, 2)):
        x = Dst(48, device)
        status = check(native, device, make_blob(segments, max_segments, head + 40, n=n), max_segments, [x])
        assert not status.any() and (x.host() != POISON).sum() in range(7 * copied - 2, 7 * copied + 1), n


def case_tiny_and_large(native, device):
    """A table row's worth beside a feats array's worth in one call — 16 bytes at a time with a head (offsets 1 mod 4 on both
    sides) — and the same pair word by word (offsets 1 and 2)."""
    max_segments, big = 8, 100003
    head = 4 + 4 * max_segments
    for rd in (1, 2):
        segments = [(0, 3, head, 100), (1, rd, head + 101, big), (0, 200, head + 104 + big, 0)]
        dsts = [Dst(256, device), Dst(big + 8, device)]
        assert not check(native, device, make_blob(segments, max_segments, head + 110 + big, seed=rd), max_segments, dsts).any()


def case_all_destinations(native, device):
    max_segments = N_DSTS
    segments, src = [], 4 + 4 * max_segments
    for d in range(N_DSTS):
        segments.append((d, d % 5, src, 40 + 17 * d))
        src += 40 + 17 * d + d % 3
    dsts = [Dst(40 + 17 * d + 8, device, lead=d % 2) for d in range(N_DSTS)]
    assert not check(native, device, make_blob(segments, max_segments, src), max_segments, dsts).any()


def refusals(max_segments, blob_words, dst_words):
    head = 4 + 4 * max_segments
    return dict(dst_too_large=(N_DSTS, 0, head, 4), dst_negative=(-1, 0, head, 4), null_destination=(1, 0, head, 4),
                negative_words=(0, 0, head, -1), source_past_the_blob=(0, 0, blob_words - 3, 4), source_in_the_header=(0, 0, head - 1, 4),
                source_offset_negative=(0, 0, -4, 4), destination_past_the_end=(0, dst_words - 3, head, 4), dst_off_negative=(0, -1, head, 4),
                huge_words=(0, 0, head, 2 ** 31 - 1), huge_offsets=(0, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))


def case_refusals(native, device):
    """Every refusal writes nothing for its segment and sets its status word; the neighbours in the same call are copied."""
    max_segments, words = 16, 4 + 4 * 16 + 64
    head = 4 + 4 * max_segments
    kinds = refusals(max_segments, words, 64)
    good = [(0, 8, head + 8, 16), (2, 30, head + 32, 20)]
    for name, bad in kinds.items():
        dsts = [Dst(64, device), None, Dst(64, device)]
        status = check(native, device, make_blob([good[0], bad, good[1]], max_segments, words), max_segments, dsts)
        assert status.tolist() == [0, 1, 0] + [0] * (max_segments - 3), name
        assert (dsts[0].host() != POISON).sum() >= 15 and (dsts[2].host() != POISON).sum() >= 19, name
    dsts = [Dst(64, device), None, Dst(64, device)]
    status = check(native, device, make_blob([good[0]] + list(kinds.values()) + [good[1]], max_segments, words), max_segments, dsts)
    assert status.tolist() == [0] + [1] * len(kinds) + [0] * (max_segments - len(kinds) - 1)
    # the edges that are still inside: a source that ends at blob_words, a destination that ends at dst_words, both of no words
    edge = [(0, 60, words - 4, 4), (2, 64, words, 0), (2, 0, head, 0)]
    assert not check(native, device, make_blob(edge, max_segments, words), max_segments, [Dst(64, device), None, Dst(64, device)]).any()
    # blob_words smaller than the buffer: the source range is held against what the call says
    status = check(native, device, make_blob([(0, 0, head, 8), (0, 8, head + 4, 8)], max_segments, words), max_segments, [Dst(64, device)],
                   blob_words=head + 8)
    assert status[:2].tolist() == [0, 1]


def case_two_launches_are_bit_identical(native, device):
    max_segments = 8
    head = 4 + 4 * max_segments
    segments = [(0, 1, head + 2, 3000), (1, 0, head + 3004, 513), (0, 3002, head + 3600, 77)]
    blob = make_blob(segments, max_segments, head + 3700)
    runs = []
    for _ in range(2):
        dsts = [Dst(3100, device), Dst(600, device, lead=1)]
        status = launch(native, device, blob, max_segments, dsts)
        runs.append([status.tobytes()] + [x.host().tobytes() for x in dsts])
    assert runs[0] == runs[1]


def case_err_arg(native, device):
    """Every MST_ERR_ARG case; a refused call enqueues nothing: destination and status stay as they were."""
    from style import _native as nat
    max_segments = 4
    head = 4 + 4 * max_segments
    blob = torch.from_numpy(make_blob([(0, 0, head, 8)], max_segments, head + 8)).to(device)
    x = Dst(16, device)
    status = torch.full((max_segments,), 1234, dtype=torch.int32, device=device)
    table = nat.AdmitDsts([(x.addr, x.words)])
    call = native.lib.mst_store_admit
    good = dict(blob=blob.data_ptr(), blob_words=head + 8, max_segments=max_segments, dst=ctypes.byref(table.ptr), dst_words=ctypes.byref(table.words),
                status=status.data_ptr(), stream=_stream(device))
    bad = [dict(blob=None), dict(dst=None), dict(dst_words=None), dict(status=None), dict(max_segments=0), dict(max_segments=-1),
           dict(blob_words=head - 1), dict(blob_words=0), dict(blob_words=-5), dict(max_segments=2 ** 31 - 1)]
    for kw in bad:
        assert call(*dict(good, **kw).values()) == -1, kw     # MST_ERR_ARG
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()
    assert (x.host() == POISON).all() and (status.cpu() == 1234).all()
    assert call(*good.values()) == 0
    assert (x.host() != POISON).sum() >= 7 and status.cpu().tolist() == [0, 0, 0, 0]


CASES = [case_lengths_and_alignment, case_more_segments_than_one_round, case_segment_counts, case_tiny_and_large, case_all_destinations,
         case_refusals, case_two_launches_are_bit_identical, case_err_arg]


# ---- the ring store
_clips = {}


def clip(k, C, R, T, percussion=True, density=.05):
    """A synthetic SparseClip in pageable memory, made once per argument list."""
    from style.data import SparseClip, sparsify
    key = (k, C, R, T, percussion, density)
    if key not in _clips:
        c = synth_clip(600 + k, C, R, T, True, density=density, bpm=70 + 3 * k)
        _clips[key] = SparseClip(c['mode'], c['bpm'], sparsify(c['pitched'], pin=False), c['instruments_features'],
                                 sparsify(c['unpitched'], pin=False) if percussion else None, bpm_target=90 + k, pin=False)
    return _clips[key]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def snapshot(store):
    """Pools, tables and bookkeeping of a ring store, for 'nothing changed' comparisons."""
    songs = [None if s is None else {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in store.songs]
    return dict(pools={n: (bits(p.cells).clone(), bits(p.feats).clone(), p.cells.data_ptr(), p.feats.data_ptr()) for n, p in store.pools.items()},
                tables={key: (bits(b['table']).clone(), list(b['songs']), list(b['free']), b['rows']) for key, b in store.buckets.items()},
                songs=songs, resident=store.resident(), heads=dict(store._heads), silent=set(store._silent), n=len(store))


def same_snapshot(a, b):
    same = lambda x, y: all(torch.equal(p, q) if torch.is_tensor(p) else p == q for p, q in zip(x, y))
    return (a['pools'].keys() == b['pools'].keys() and all(same(a['pools'][n], b['pools'][n]) for n in a['pools'])
            and a['tables'].keys() == b['tables'].keys() and all(same(a['tables'][k], b['tables'][k]) for k in a['tables'])
            and all(a[k] == b[k] for k in ('songs', 'resident', 'heads', 'silent', 'n')))


def verify(store, sources, capacity, resident):
    """The invariants after a step.  `sources`: id -> the SparseClip that was admitted (as drop_silent leaves it)."""
    from style.data import WindowBatch, get_used_instruments
    live = store.resident()
    n = len(store)
    assert n == len(sources) and len(live) <= resident and live == sorted(live)
    assert live == list(range(n))[n - len(live):], 'the evicted songs are not exactly the oldest'
    for i in range(n):
        assert store.evicted(i) == (i not in live) and (store.songs[i] is None) == (i not in live)
    assert sorted(s for b in store.buckets.values() for s in b['songs']) == live
    for name, nfeat in (('pitched', 5), ('unpitched', 2)):
        ranges = sorted(store.songs[i][name] for i in live if store.songs[i][name] is not None)
        for (first, count), nxt in zip(ranges, ranges[1:] + [(capacity, 0)]):
            assert first % 4 == 0 and 0 <= first and first + count <= nxt[0], (name, ranges)
        assert store.pools[nfeat].cells.numel() == capacity and tuple(store.pools[nfeat].feats.shape) == (capacity, nfeat)
    for key, b in store.buckets.items():
        rows = [store.songs[i]['row'] for i in b['songs']]
        assert len(set(rows)) == len(rows) and not set(rows) & set(b['free']) and max(rows + [-1]) < b['table'].shape[0]
        assert set(b['views']) <= set(b['songs'])
    assert all(i in live for i, _ in store._silent)
    for i in live:
        src, s = sources[i], store.songs[i]
        for name, nfeat, roll in (('pitched', 5, src.pitched_channels), ('unpitched', 2, src.unpitched_channels)):
            if roll is None:
                assert s[name] is None
                continue
            first, count = s[name]
            assert count == roll.count
            assert torch.equal(store.pools[nfeat].cells[first:first + count].cpu(), roll.cells)
            assert torch.equal(bits(store.pools[nfeat].feats[first:first + count]), bits(roll.feats))
        views = store.small_inputs(WindowBatch(s['C'], 1, s['T'], s['percussion'], [i], [0]))
        want = (src.mode, src.bpm, src.instruments_features, get_used_instruments(src.instruments_features, src.unpitched_channels),
                torch.tensor([float(src.bpm_target)]))
        assert len(views) == 5 and all(torch.equal(bits(v), bits(w.reshape(-1))) for v, w in zip(views, want)), i


SMALL, MEDIUM, BIG = (1, 2, 1), (2, 3, 1), (2, 4, 2)        # (C, R, T)
RESIDENT = 6


def script():
    """The scripted sequence: [(what, clips)] and the ring capacity that makes song 3's pitched records end exactly at it."""
    from style.data import ring_place
    first = [clip(0, *MEDIUM), clip(1, *SMALL), clip(2, *MEDIUM)]
    exact = clip(3, *MEDIUM)
    head = 0
    for c in first:
        _, head = ring_place(head, c.pitched_channels.count, 1 << 30)
    capacity = ring_place(head, 0, 1 << 30)[0] + exact.pitched_channels.count
    from style.data import SparseClip, SparseRoll
    some = clip(20, *SMALL)
    silent = SparseRoll(some.pitched_channels.cells, torch.zeros_like(some.pitched_channels.feats), some.pitched_channels.shape, pin=False)
    nothing = SparseClip(some.mode, some.bpm, silent, some.instruments_features, some.unpitched_channels, some.bpm_target, pin=False)
    steps = [('group of three', first), ('ends exactly at capacity', [exact]), ('wraps the pitched pool', [clip(4, *SMALL)]),
             ('evicts several', [clip(5, *BIG)]), ('too large', [clip(6, 2, 5, 2, density=.12)]),
             ('too large inside a group', [clip(7, *SMALL), clip(6, 2, 5, 2, density=.12)]), ('no pitched notes', [nothing]),
             ('no percussion', [clip(8, 2, 2, 1, percussion=False)])]
    for k in range(9, 21):                                    # on until the unpitched pool has wrapped as well
        steps.append(('more', [clip(k, *(MEDIUM if k % 3 else BIG))] + ([clip(30 + k, *SMALL)] if k % 4 == 0 else [])))
    return steps, capacity


def run_script(device, native=None, after_step=None):
    """The scripted sequence on a ring store on `device` (with `native`, a store on the host copies through mst_store_admit);
    `verify` after every step; `after_step(store, sources)` as well.  Returns the store."""
    import pytest
    from style.data import SongStore
    steps, capacity = script()
    store = SongStore(device, capacity=capacity, resident=RESIDENT)
    store.admit_native = native
    ptrs = [t.data_ptr() for p in store.pools.values() for t in (p.cells, p.feats)]
    sources, seen = {}, set()
    rows_freed, rows_reused = set(), False
    for what, clips in steps:
        before, live_before = snapshot(store), store.resident()
        if what in ('too large', 'too large inside a group', 'no pitched notes'):
            with pytest.raises(ValueError):
                store.admit(clips)
            assert same_snapshot(before, snapshot(store)), what
            seen.add(what)
        else:
            ids = store.admit(clips)
            assert ids == list(range(before['n'], before['n'] + len(clips)))
            for i, c in zip(ids, clips):
                sources[i] = c.drop_silent()
            gone = [i for i in live_before if store.evicted(i)]
            for i in gone:
                rows_freed.add((before['songs'][i]['key'], before['songs'][i]['row']))
            for i in ids:
                s = store.songs[i]
                if s is None:
                    continue
                rows_reused |= (s['key'], s['row']) in rows_freed
                if i and s['pitched'][0] == 0:
                    seen.add('pitched wrap')
                if i and s['unpitched'] is not None and s['unpitched'][0] == 0 and before['heads'][2] > 0:
                    seen.add('unpitched wrap')
                if sum(s['pitched']) == capacity:
                    seen.add('ends exactly at capacity')
            if len(gone) >= 2 and len(clips) == 1:
                seen.add('evicts several')
            if len(clips) == 3:
                seen.add('group of three')
        store.check()
        verify(store, sources, capacity, RESIDENT)
        if after_step is not None:
            after_step(store, sources)
    assert seen == {'too large', 'too large inside a group', 'no pitched notes', 'pitched wrap', 'unpitched wrap', 'ends exactly at capacity',
                    'evicts several', 'group of three'}, seen
    assert rows_reused, 'no table row was reused'
    assert len(set(range(len(store)))) == len(store) and len(store) == len(sources)
    assert ptrs == [t.data_ptr() for p in store.pools.values() for t in (p.cells, p.feats)], 'a pool moved'
    return store


def crops(native, store, song, bars=2):
    """Every `bars`-bar window of a resident song cropped by mst_clip_window out of the store: (pitched, unpitched | None) bits."""
    from style.data import WindowBatch
    s = store.songs[song]
    K = s['R'] - bars + 1
    batch = WindowBatch(s['C'], bars, s['T'], s['percussion'], [song] * K, list(range(K)))
    win = np.zeros((2, K, 4), np.int32)
    store.describe(batch, win)
    win = torch.from_numpy(win).to(store.device)
    out = []
    for row, nfeat, ch, notes in ((0, 5, s['C'], 56), (1, 2, 1, 47)):
        if row and not s['percussion']:
            out.append(None)
            continue
        x = torch.full((K, ch, bars, s['T'] * 10 * notes, nfeat), float('nan'), device=store.device)
        native.clip_window(store.pools[nfeat].cells, store.pools[nfeat].feats, win[row], x, K, ch, bars, s['T'] * 10 * notes, nfeat,
                           _stream(store.device))
        out.append(bits(x))
    return out


def case_ring_crops_equal_the_append_only_store(native, device):
    """After every step of the script: every 2-bar window of every resident song, cropped out of the ring store, equals — as
    int32 bits — the crop out of a fresh append-only store holding the same songs; `check` is clean (run_script calls it)."""
    from style.data import SongStore

    def after(store, sources):
        live = store.resident()
        twin = SongStore(device, capacity=64)
        ids = {i: twin.add(sources[i]) for i in live}
        for i in live:
            for got, want in zip(crops(native, store, i), crops(native, twin, ids[i])):
                assert (got is None) == (want is None) and (got is None or (torch.equal(got, want) and bool((got != 0).any()))), i
    run_script(device, native, after)
