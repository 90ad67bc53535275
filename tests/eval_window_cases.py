"""Windowed evaluation cases shared by the CPU-interpreter tests and the -m gpu tests: mst_window_inputs, mst_eval_accumulate and
their composition with mst_clip_window and mst_eval_iteration at the C ABI.  Both builds drive the SAME C ABI; only the library
(hipsim vs hipcc/gfx950) and the device differ.  Every comparison is bit equality: a gather is a copy, and a left-to-right float64
sum has one answer — the one a Python loop of np.float64 additions in the same order gives.  There is no tolerance to choose.

The songs are those of tests/test_gpu_clip_window.py (C = 2, T = 2, percussion, 2 / 5 / 3 / 4 / 3 bars, each with its own mode, bpm
and instruments) and the windows are 2 bars: the smallest shapes where a window starts inside a song, a table row differs per
clip and a batch needs padding."""
import numpy as np
import torch

import eval_cases as ec
import parity_cases as pc
from simutil import make_dims
from style import _native as nat
from tools.synth import synth_clip

ERR_ARG = -1
C, T, BARS = 2, 2, 2
SONG_BARS = (2, 5, 3, 4, 3)
POISON = 0x7fc00abc                      # a NaN that no kernel writes: a float that still holds it was not written
QNAN = 0x7fc00000                        # what mst_window_inputs writes for a row outside the table
N_LOSSES, W, ACC = nat.N_LOSSES, nat.METRIC_WORDS, 41
U0, U1 = 7, 11                           # the unpitched leaves MST_L_U_TOTAL .. MST_L_U_DURATION
_cache = {}


def stream(device):
    return nat.current_stream(device)


# ---- the songs
def songs():
    """Five songs of 2 to 5 bars (C = 2, T = 2, with percussion), each with its own mode, bpm and instruments: the recipe of
    tests/test_gpu_clip_window.py.  Computed once."""
    if 'songs' not in _cache:
        out = []
        for k, R in enumerate(SONG_BARS):
            clip = synth_clip(300 + k, C, R, T, True, density=.05, bpm=80 + 11 * k)
            if k % 2:
                clip['mode'] = torch.tensor([[0., 1.]])
            feats = torch.zeros_like(clip['instruments_features'])
            for c in range(C):
                feats[0, c, (3 * k + c) % 40] = 1.
                feats[0, c, 40 + (k + c) % 11] = 1.
            clip['instruments_features'] = feats
            used = (feats[:, :, :40].sum(1) > 0).float()
            clip['used_instruments'] = torch.cat([used, torch.ones(1, 1)], 1)
            out.append(clip)
        _cache['songs'] = out
    return _cache['songs']


def make_store(device, clips=None):
    from style.data import SongStore, SparseClip, sparsify
    pin = torch.device(device).type != 'cpu'
    store = SongStore(device, capacity=256)
    for clip in songs() if clips is None else clips:
        store.add(SparseClip(clip['mode'], clip['bpm'], sparsify(clip['pitched'], pin=pin), clip['instruments_features'],
                             sparsify(clip['unpitched'], pin=pin), bpm_target=clip['bpm_int'], pin=pin))
    return store


def cropped(batch, clips=None):
    """The batch's clips cropped on the host: [(pitched (1, C, BARS, T, 10, 56, 5), unpitched (1, 1, BARS, T, 10, 47, 2))]."""
    clips = songs() if clips is None else clips
    return [(clips[s]['pitched'][:, :, r0:r0 + batch.bars].contiguous(), clips[s]['unpitched'][:, :, r0:r0 + batch.bars].contiguous())
            for s, r0 in zip(batch.songs.tolist(), batch.r0s.tolist())]


# ---- mst_window_inputs
LENS = (2, 1, 102, 41, 1)               # mode, bpm, instrument features (C = 2), used instruments, bpm target
SRC = (0, 2, 3, 105, 146)
DST = (300, 7, 20, 130, 180)            # disjoint, out of order, gaps between them
ROW_FLOATS, STRIDE = 147, 311           # an odd clip stride


def table(rows=6, seed=0):
    """`rows` x 147 words of arbitrary bit patterns — signalling and payload NaNs, infinities, -0.0 and denormals among them: a
    bit copy must carry them all."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 2 ** 32, (rows, ROW_FLOATS), dtype=np.uint64).astype(np.uint32)
    t[0, :6] = (0x7fa00001, 0xffc12345, 0x80000000, 0x00000001, 0x7f800000, 0xff800000)
    return t


def gather(buf, base, tab, rows, fields, stride):
    """The numpy gather into a copy of the uint32 buffer `buf`, whose workspace starts at word `base`."""
    out = buf.copy()
    for k, row in enumerate(rows):
        for src, n, dst in fields:
            at = base + dst + k * stride
            out[at:at + n] = tab[row, src:src + n] if 0 <= row < len(tab) else QNAN
    return out


def run_inputs(native, device, tab, rows, fields, stride, lead=0, guard=16, table_rows=None):
    """mst_window_inputs into a poisoned buffer: `guard` floats, then the workspace `lead` floats further on, then `guard`
    floats.  Returns (the buffer before, the buffer after, the workspace's first word) as uint32 numpy."""
    K = len(rows)
    span = max(dst + n for _, n, dst in fields) + (K - 1) * stride
    buf = torch.full((guard + lead + span + guard,), POISON, dtype=torch.int32, device=device)
    before = buf.cpu().numpy().view(np.uint32).copy()
    dtab = torch.from_numpy(tab.view(np.int32).copy()).to(device)
    drows = torch.tensor(rows, dtype=torch.int32, device=device)
    native.window_inputs(dtab.data_ptr(), len(tab) if table_rows is None else table_rows, tab.shape[1], drows, K, fields, stride,
                         buf.data_ptr() + 4 * (guard + lead), stream(device))
    after = buf.cpu().numpy().view(np.uint32).copy()
    assert np.array_equal(dtab.cpu().numpy().view(np.uint32), tab), 'the table is read only'
    return before, after, guard + lead


def inputs_check(native, device, rows, lead=0, fields=None, stride=STRIDE, tab=None):
    tab = table() if tab is None else tab
    fields = list(zip(SRC, LENS, DST)) if fields is None else fields
    before, after, base = run_inputs(native, device, tab, rows, fields, stride, lead)
    want = gather(before, base, tab, rows, fields, stride)
    assert np.array_equal(after, want), np.flatnonzero(after != want)[:8]
    named = len({dst + k * stride + i for k in range(len(rows)) for _, n, dst in fields for i in range(n)})
    assert (after != POISON).sum() == named                 # everything named was written, nothing else was
    return after


def case_inputs_gather(native, device):
    """K = 1 and K = 5 with a repeated row, field lengths 2, 1, 102, 41, 1, destination at an even and at odd float offsets."""
    assert sum(LENS) == ROW_FLOATS
    for lead in (0, 1, 3):
        inputs_check(native, device, [4], lead)
        inputs_check(native, device, [3, 0, 3, 1, 5], lead)
    inputs_check(native, device, [2, 2, 2], stride=0, fields=[(5, 9, 0)])       # clip_stride = 0 is allowed: the clips coincide


def case_inputs_more_than_one_chunk(native, device):
    """A row of 2500 floats placed as three fields (1024 + 1 and 1475): a clip's fields span three workgroups."""
    rng = np.random.default_rng(3)
    tab = rng.integers(0, 2 ** 32, (3, 2500), dtype=np.uint64).astype(np.uint32)
    fields = [(0, 1024, 3000), (1024, 1, 10), (1025, 1475, 100), (7, 0, 5)]      # and one of length 0, which names nothing
    inputs_check(native, device, [2, 0, 1, 2], lead=1, fields=fields, stride=4099, tab=tab)


def case_inputs_rows_outside_the_table(native, device):
    """A row index = table_rows, one far beyond and negative ones: quiet NaNs in that clip's fields only."""
    tab = table()
    for rows in ([1, len(tab), 0], [-1, 2, -2 ** 31, 2 ** 31 - 1]):
        after = inputs_check(native, device, rows, lead=1, tab=tab)
        assert (after == QNAN).sum() >= ROW_FLOATS * sum(not 0 <= r < len(tab) for r in rows)
    # table_rows says where the table ends, not the buffer: a row that exists in memory but not in the table is not read
    fields = list(zip(SRC, LENS, DST))
    before, after, base = run_inputs(native, device, tab, [3, 1], fields, STRIDE, table_rows=3)
    assert np.array_equal(after, gather(before, base, tab[:3], [3, 1], fields, STRIDE))


def case_inputs_err_arg(native, device):
    """Every MST_ERR_ARG case; a refused call writes nothing."""
    tab = torch.from_numpy(table().view(np.int32).copy()).to(device)
    rows = torch.tensor([1, 2], dtype=torch.int32, device=device)
    ws = torch.full((700,), POISON, dtype=torch.int32, device=device)
    call = native.lib.mst_window_inputs
    F = lambda fields: nat.RowFields.of(fields)
    good_fields = list(zip(SRC, LENS, DST))

    def args(**kw):
        a = dict(table=tab.data_ptr(), table_rows=6, row_floats=ROW_FLOATS, rows=rows.data_ptr(), n_clips=2, fields=F(good_fields),
                 clip_stride=STRIDE, ws=ws.data_ptr(), stream=None)
        a.update(kw)
        f = a['fields']
        return (a['table'], a['table_rows'], a['row_floats'], a['rows'], a['n_clips'], None if f is None else nat.C.byref(f),
                a['clip_stride'], a['ws'], a['stream'])
    wrong_n = [F(good_fields) for _ in range(3)]
    wrong_n[0].n, wrong_n[1].n, wrong_n[2].n = 0, 9, -1
    bad = [args(table=None), args(rows=None), args(fields=None), args(ws=None), args(n_clips=0), args(n_clips=-3), args(table_rows=0),
           args(table_rows=-1), args(row_floats=0), args(row_floats=-147), args(clip_stride=-1), args(fields=wrong_n[0]),
           args(fields=wrong_n[1]), args(fields=wrong_n[2]), args(fields=F([(-1, 2, 0)])), args(fields=F([(0, -2, 0)])),
           args(fields=F([(0, 2, -1)])), args(fields=F([(146, 2, 0)])), args(fields=F([(0, 148, 0)])), args(row_floats=146),
           args(fields=F([(0, 2, 0), (2 ** 31 - 1, 1, 4)]))]
    for a in bad:
        assert call(*a) == ERR_ARG, a
    assert (ws.cpu().numpy().view(np.uint32) == POISON).all()                   # nothing was launched
    assert call(*args(stream=stream(device))) == 0
    assert (ws.cpu().numpy().view(np.uint32) != POISON).sum() == 2 * ROW_FLOATS


# ---- mst_eval_accumulate
def batch_values(K, channels, seed, no_percussion=(), nan_total=()):
    """Random losses (K x 15 float32) and metrics (K x (channels + 2) x 8 float64 — fractions, so that every addition rounds).
    Clips of `no_percussion` have NaN unpitched leaves, clips of `nan_total` a NaN total."""
    rng = np.random.default_rng(seed)
    losses = (rng.random((K, N_LOSSES)) * 3 + .01).astype(np.float32)
    metrics = rng.random((K, channels + 2, W)) * 1000. + rng.random((K, channels + 2, W)) * 1e-7
    for k in no_percussion:
        losses[k, U0:U1] = np.nan
    for k in nan_total:
        losses[k, 0] = np.nan
    return losses, metrics


def fold(acc, losses, metrics, live):
    """The sequential np.float64 loop the header promises the bits of."""
    acc = [np.float64(x) for x in acc]
    K, per = len(losses), metrics.shape[1]
    channels = per - 2
    n = K if live is None else min(max(live, 0), K)
    one = np.float64(1.)
    with np.errstate(invalid='ignore'):
        for k in range(n):
            has_u = not np.isnan(losses[k, U0])
            acc[0] = acc[0] + one
            if has_u:
                acc[1] = acc[1] + one
            for i in range(N_LOSSES):
                if has_u or not U0 <= i < U1:
                    acc[2 + i] = acc[2 + i] + np.float64(losses[k, i])
            for j in range(W):
                for c in range(channels):
                    acc[17 + j] = acc[17 + j] + np.float64(metrics[k, c, j])
                acc[25 + j] = acc[25 + j] + np.float64(metrics[k, channels, j])
                term = np.float64(metrics[k, channels + 1, j])
                acc[33 + j] = acc[33 + j] + (term + one if j == W - 1 else term)
    return np.array(acc, dtype=np.float64)


def run_accumulate(native, device, acc0, losses, metrics, live, guard=4, calls=1):
    K, channels = len(losses), metrics.shape[1] - 2
    buf = torch.full((ACC + 2 * guard,), float('nan'), dtype=torch.float64, device=device)
    buf[guard:guard + ACC] = torch.from_numpy(np.asarray(acc0, dtype=np.float64))
    before = buf.cpu().clone()
    dl, dm = torch.from_numpy(losses).to(device), torch.from_numpy(metrics).to(device)
    dlive = None if live is None else torch.tensor([live], dtype=torch.int32, device=device)
    for _ in range(calls):
        native.eval_accumulate(dl, dm, K, channels, dlive, buf.data_ptr() + 8 * guard, stream(device))
    after = buf.cpu()
    assert ec.same_bits(after[:guard], before[:guard]) and ec.same_bits(after[-guard:], before[-guard:]), 'a store outside acc'
    assert ec.same_bits(dl.cpu(), torch.from_numpy(losses)) and ec.same_bits(dm.cpu(), torch.from_numpy(metrics))
    return after[guard:guard + ACC].numpy().copy()


def same_doubles(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def case_accumulate_live(native, device):
    """live = NULL, 0, 1, K, K + 3, -2 against the sequential loop, from a zero and from a non-zero accumulator; K = 11 takes the
    kernel's look-ahead past one round, with a ragged last one."""
    for K, channels in ((5, 2), (11, 3), (1, 1)):
        losses, metrics = batch_values(K, channels, seed=K)
        start = np.random.default_rng(9).random(ACC) * 50.
        start[3] = -0.                                                # a word without terms keeps its bits, -0.0 too
        for acc0 in (np.zeros(ACC), start):
            for live, counted in ((None, K), (0, 0), (1, 1), (K, K), (K + 3, K), (-2, 0)):
                got = run_accumulate(native, device, acc0, losses, metrics, live)
                want = fold(acc0, losses, metrics, live)
                assert same_doubles(got, want), (K, live, np.flatnonzero(got != want))
                if not acc0.any():
                    assert got[0] == counted, (live, got[0])
                if counted == 0:
                    assert same_doubles(got, acc0)


def case_accumulate_more_than_one_stretch(native, device):
    """The kernel walks the batch in stretches of 546 loss rows and of 512 records: 600 clips of one channel are two and four of
    them, 70 clips of nine channels two stretches of records that begin inside a clip (512 = 46 * 11 + 6)."""
    for K, channels, lives in ((600, 1, (None, 547, 546, 171)), (70, 9, (None, 47))):
        losses, metrics = batch_values(K, channels, seed=K, no_percussion=(0, 5, K - 1))
        start = np.random.default_rng(K).random(ACC)
        for live in lives:
            got = run_accumulate(native, device, start, losses, metrics, live)
            want = fold(start, losses, metrics, live)
            assert same_doubles(got, want), (K, live, np.flatnonzero(got != want))


def case_accumulate_percussion_and_nan(native, device):
    """Clips whose unpitched leaves are NaN: [1] and those four sums do not move for them.  A NaN total leaf propagates."""
    K = 5
    losses, metrics = batch_values(K, 2, seed=21, no_percussion=(0, 3))
    got = run_accumulate(native, device, np.zeros(ACC), losses, metrics, None)
    assert same_doubles(got, fold(np.zeros(ACC), losses, metrics, None))
    assert got[0] == 5 and got[1] == 3 and np.isfinite(got).all()
    # nobody has percussion: the four sums and [1] keep the bits they had
    losses, metrics = batch_values(K, 2, seed=22, no_percussion=range(K))
    start = np.arange(ACC, dtype=np.float64) + .25
    got = run_accumulate(native, device, start, losses, metrics, None)
    assert same_doubles(got, fold(start, losses, metrics, None))
    assert same_doubles(got[[1] + [2 + i for i in range(U0, U1)]], start[[1] + [2 + i for i in range(U0, U1)]])
    # a NaN total is a real one
    losses, metrics = batch_values(K, 2, seed=23, nan_total=(2,))
    got = run_accumulate(native, device, np.zeros(ACC), losses, metrics, None)
    assert same_doubles(got, fold(np.zeros(ACC), losses, metrics, None))
    assert np.isnan(got[2]) and np.isfinite(np.delete(got, 2)).all()
    got = run_accumulate(native, device, np.zeros(ACC), losses, metrics, 2)    # ... when its clip is counted
    assert np.isfinite(got).all()


def case_accumulate_twice(native, device):
    """Two calls in a row accumulate: the second starts from what the first left."""
    losses, metrics = batch_values(4, 2, seed=31, no_percussion=(1,))
    got = run_accumulate(native, device, np.zeros(ACC), losses, metrics, 3, calls=2)
    once = fold(np.zeros(ACC), losses, metrics, 3)
    assert same_doubles(got, fold(once, losses, metrics, 3)) and got[0] == 6 and got[1] == 4 and got[40] >= 6


def case_accumulate_err_arg(native, device):
    losses, metrics = batch_values(3, 2, seed=41)
    dl, dm = torch.from_numpy(losses).to(device), torch.from_numpy(metrics).to(device)
    acc = torch.full((ACC + 2,), float('nan'), dtype=torch.float64, device=device)
    live = torch.tensor([3], dtype=torch.int32, device=device)
    call = native.lib.mst_eval_accumulate
    ok = (dl.data_ptr(), dm.data_ptr(), 3, 2, live.data_ptr(), acc.data_ptr())
    bad = [(0, None), (1, None), (5, None), (2, 0), (2, -1), (3, 0), (3, -2), (1, dm.data_ptr() + 4), (5, acc.data_ptr() + 4)]
    for at, value in bad:
        a = ok[:at] + (value,) + ok[at + 1:]
        assert call(*a, None) == ERR_ARG, a
    assert torch.isnan(acc.cpu()).all()                                         # nothing was launched
    acc.zero_()
    assert call(*ok[:4], None, acc.data_ptr(), stream(device)) == 0              # a null `live` is allowed: all clips
    assert float(acc.cpu()[0]) == 3


# ---- the composition at the C ABI
def case_composition(native, device, K=3, gemm_tile=None):
    """crops -> mst_window_inputs -> mst_eval_iteration -> mst_eval_accumulate on a Plan(clips = K) at SMALL widths, against the
    same plan fed host-cropped dense clips and set_inputs per clip: per-clip losses, predictions and metrics identical in every
    bit, and acc the numpy fold of them."""
    from style.data import WindowBatch
    store = make_store(device)
    picks = [(1, 2), (3, 1), (0, 0), (4, 1), (1, 3), (2, 0), (3, 2), (1, 0)][:K]           # windows that start inside a song
    batch = WindowBatch(C, BARS, T, True, [s for s, _ in picks], [r for _, r in picks])
    plan = nat.Plan(native, make_dims(pc.SMALL, C, BARS, T, True, clips=K), device, gemm_tile=gemm_tile)
    params = ec.eval_params(native, make_dims(pc.SMALL, C, BARS, T, True)).to(device)
    bucket = store.buckets[(C, T, True)]
    tab = bucket['table']
    names = ('mode', 'bpm', 'instr', 'used_instruments', 'bpm_target')
    fields = [(a, b - a, plan.slot(n)[0]) for n, (a, b) in zip(names, bucket['fields'])]
    assert [n for _, n, _ in fields] == list(LENS) and all(plan.slot(n)[2] == l for n, l in zip(names, LENS))
    # the device path
    win = torch.zeros(2, K, 4, dtype=torch.int32)
    store.describe(batch, win.numpy())
    win = win.to(device)
    rows = torch.tensor([store.songs[s]['row'] for s in batch.songs.tolist()], dtype=torch.int32, device=device)
    assert len(set(rows.tolist())) > 1
    xp = torch.full((K, C, BARS, T, 10, 56, 5), float('nan'), device=device)
    xu = torch.full((K, 1, BARS, T, 10, 47, 2), float('nan'), device=device)
    ws = plan.new_ws()
    ec._poison(plan, ws, True)
    for k in range(K):
        for n in names:
            plan.view(n, ws=ws, clip=k).fill_(float('nan'))
    native.clip_window(store.pools[5].cells, store.pools[5].feats, win[0], xp, K, C, BARS, T * 560, 5, stream(device))
    native.clip_window(store.pools[2].cells, store.pools[2].feats, win[1], xu, K, 1, BARS, T * 470, 2, stream(device))
    native.window_inputs(tab, tab.shape[0], tab.shape[1], rows, K, fields, plan.clip_stride, ws, stream(device))
    losses = torch.full((K, N_LOSSES), -7., device=device)
    metrics = torch.full((K, C + 2, W), float('nan'), dtype=torch.float64, device=device)
    plan.eval_iteration(params, xp, xu, losses, metrics, ws=ws)
    live = torch.tensor([K - 1], dtype=torch.int32, device=device)
    acc = torch.zeros(ACC, dtype=torch.float64, device=device)
    native.eval_accumulate(losses, metrics, K, C, live, acc, stream(device))
    # the host path: the same plan, dense clips cropped on the host, set_inputs per clip
    dense = cropped(batch)
    hp, hu = torch.cat([p for p, _ in dense]).to(device), torch.cat([u for _, u in dense]).to(device)
    assert ec.same_bits(xp, hp.reshape(xp.shape)) and ec.same_bits(xu, hu.reshape(xu.shape))
    ws2, losses2, metrics2 = ec._run_eval(plan, params, hp, hu, [songs()[s] for s in batch.songs.tolist()], True)
    assert ec.same_bits(losses, losses2) and ec.same_bits(metrics, metrics2)
    assert torch.isfinite(losses).all() and not ec.same_bits(losses[0], losses[1])
    for k in range(K):
        for n in names + ec.PRED_NAMES:
            assert ec.same_bits(plan.view(n, ws=ws, clip=k), plan.view(n, ws=ws2, clip=k)), (n, k)
    want = fold(np.zeros(ACC), losses2.cpu().numpy(), metrics2.cpu().numpy(), K - 1)
    assert same_doubles(acc.cpu().numpy(), want) and want[0] == K - 1 and want[1] == K - 1 and want[40] == K - 1
    assert ec.counts_not_trivial(want[17:25]) and ec.counts_not_trivial(want[25:33])
    return plan.gemm_tile


KERNEL_CASES = [case_inputs_gather, case_inputs_more_than_one_chunk, case_inputs_rows_outside_the_table, case_inputs_err_arg,
                case_accumulate_live, case_accumulate_more_than_one_stretch, case_accumulate_percussion_and_nan, case_accumulate_twice, case_accumulate_err_arg]
