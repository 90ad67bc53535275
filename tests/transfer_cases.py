"""Batched style transfer cases shared by the CPU-interpreter tests and the -m gpu tests: mst_clip_gather, mst_rolls_count /
mst_rolls_compact, mst_style_sums and their composition with mst_clip_window, mst_window_inputs, mst_forward's stage masks,
mst_clip_scatter and mst_roll_metrics at the C ABI.  Both builds drive the SAME C ABI; only the library (hipsim vs hipcc/gfx950)
and the device differ.  Every comparison is bit equality: a gather is a copy, a compaction has one answer, and a left-to-right
float64 sum has one answer — the one a Python loop of np.float64 additions in the same order gives.  There is no tolerance to
choose.

The songs are those of tests/eval_window_cases.py (C = 2, T = 2, percussion, 2-bar windows, SMALL widths)."""
import numpy as np
import torch

import eval_cases as ec
import eval_window_cases as wc
import parity_cases as pc
from oracle import style_oracle as so
from simutil import make_dims
from style import _native as nat

ERR_ARG = -1
POISON, QNAN = wc.POISON, wc.QNAN
S = 1024                                 # cells of a roll one workgroup owns (ROLL_SLICE, csrc/loss_optim.hip)
NONZERO, HARD = nat.ROLL_NONZERO, nat.ROLL_HARD
C, T, BARS = wc.C, wc.T, wc.BARS
DONORS = [2, 0, 0]
stream = wc.stream


def words(t):
    """A device tensor's bits as uint32 numpy."""
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32).copy()


def poisoned(n, device):
    return torch.full((n,), POISON, dtype=torch.int32, device=device)


def odd(n):
    return n | 1


# ---- mst_clip_gather
def source(rows, stride, length, seed=0):
    """The uint32 words of `rows` runs of `length` floats, `stride` apart: arbitrary bit patterns, NaNs of every kind among them."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 2 ** 32, (rows - 1) * stride + length, dtype=np.uint64).astype(np.uint32)
    src[:min(6, len(src))] = (0x7fa00001, 0xffc12345, 0x80000000, 0x00000001, 0x7f800000, 0xff800000)[:min(6, len(src))]
    return src


def gathered(before, base, src, src_rows, src_stride, dst_stride, idx, K, length):
    out = before.copy()
    for k in range(K):
        row = k if idx is None else idx[k]
        at = base + k * dst_stride
        out[at:at + length] = src[row * src_stride:row * src_stride + length] if 0 <= row < src_rows else QNAN
    return out


def gather_check(native, device, idx, K, length, src_rows=6, src_stride=None, dst_stride=None, lead=0, guard=16, buffer_rows=None):
    """mst_clip_gather into a poisoned buffer: `guard` floats, the destination `lead` floats further on, `guard` floats."""
    src_stride = odd(length + 2) if src_stride is None else src_stride
    dst_stride = odd(length + 4) if dst_stride is None else dst_stride
    src = source(src_rows if buffer_rows is None else buffer_rows, src_stride, length, seed=length + K)
    dsrc = torch.from_numpy(src.view(np.int32).copy()).to(device)
    buf = poisoned(guard + lead + (K - 1) * dst_stride + length + guard, device)
    before = words(buf)
    didx = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=device)
    native.clip_gather(dsrc, src_rows, src_stride, buf.data_ptr() + 4 * (guard + lead), dst_stride, didx, K, length, stream(device))
    after = words(buf)
    want = gathered(before, guard + lead, src, src_rows, src_stride, dst_stride, idx, K, length)
    assert np.array_equal(after, want), (K, length, lead, np.flatnonzero(after != want)[:8])
    assert (after != POISON).sum() == K * length              # everything named was written, nothing else was
    assert np.array_equal(words(dsrc), src), 'src is read only'
    return after


def case_gather_copies(native, device):
    """Every length around the lane count and past one workgroup's chunk, K = 1 and 5 with repeated rows, odd strides,
    destinations at float offsets 0, 1 and 3 from a 16-byte boundary; the identity by NULL; src_stride = 0."""
    for length in (1, 63, 64, 65, 1025, 2500):
        for K, idx in ((1, [4]), (5, [3, 0, 3, 1, 5])):
            for lead in (0, 1, 3):
                gather_check(native, device, idx, K, length, lead=lead)
            gather_check(native, device, None, K, length, lead=1)
    gather_check(native, device, [0, 2, 1], 3, 65, src_stride=0, lead=3)      # every row is the same run
    gather_check(native, device, [4, 4, 0, 2], 4, 64, dst_stride=64)          # destinations back to back


def case_gather_rows_outside(native, device):
    """An index = src_rows, far beyond and negative ones: quiet NaNs in that clip only; src_rows says where src ends."""
    for idx in ([1, 6, 0], [-1, 2, -2 ** 31, 2 ** 31 - 1], [5, 5, 5, 5, 5]):
        for length in (1, 65, 1025):
            after = gather_check(native, device, idx, len(idx), length, lead=1)
            assert (after == QNAN).sum() >= length * sum(not 0 <= r < 6 for r in idx)
    gather_check(native, device, [3, 1, 2], 3, 65, src_rows=3, buffer_rows=6)  # row 3 exists in memory, not in src
    gather_check(native, device, None, 5, 63, src_rows=3, buffer_rows=6)       # the identity past src_rows


def case_gather_err_arg(native, device):
    """Every MST_ERR_ARG case; a refused call writes nothing."""
    src = torch.from_numpy(source(6, 71, 64).view(np.int32).copy()).to(device)
    dst = poisoned(6 * 71, device)
    idx = torch.tensor([1, 0], dtype=torch.int32, device=device)
    call = native.lib.mst_clip_gather

    def args(**kw):
        a = dict(src=src.data_ptr(), src_rows=6, src_stride=71, dst=dst.data_ptr(), dst_stride=71, idx=idx.data_ptr(), n_clips=2, len=64,
                 stream=None)
        a.update(kw)
        return tuple(a[k] for k in ('src', 'src_rows', 'src_stride', 'dst', 'dst_stride', 'idx', 'n_clips', 'len', 'stream'))
    d = dst.data_ptr()
    bad = [args(src=None), args(dst=None), args(n_clips=0), args(n_clips=-2), args(src_rows=0), args(src_rows=-1), args(len=0),
           args(len=-64), args(src_stride=-1), args(dst_stride=-71), args(dst_stride=63), args(dst_stride=0),
           # the two ranges intersect: the same buffer, a destination inside the source rows, ranges that touch in one float
           args(src=d, src_rows=2), args(src=d, src_rows=2, dst=d + 4 * 71), args(src=d, src_rows=2, dst=d + 4 * (71 + 63)),
           args(src=d + 4 * (71 + 63), src_rows=2), args(src=d + 4 * 100, src_rows=1, src_stride=0, dst=d, n_clips=2),
           args(src_stride=2 ** 62), args(dst_stride=2 ** 62, n_clips=3)]
    for a in bad:
        assert call(*a) == ERR_ARG, a
    assert (words(dst) == POISON).all()                                         # nothing was launched
    assert call(*args(src=d + 4 * (71 + 64), src_rows=2, stream=stream(device))) == 0      # disjoint by one float: allowed
    assert call(*args(dst_stride=63, n_clips=1, idx=None, stream=stream(device))) == 0     # one clip has no stride
    assert call(*args(stream=stream(device))) == 0
    assert (words(dst) != POISON).sum() == 2 * 64


# ---- mst_rolls_count / mst_rolls_compact
_rolls = {}


def roll_set(n_cells, nfeat, n_rolls):
    """`n_rolls` host rolls (n_cells x nfeat float32).  Roll 0 is random at 20 % density and carries the edge cells: -0.0 and NaN
    features, velocities at .01f, nextafter(.01f) and NaN, accidentals tied at the maximum and at .1f; roll 1 is empty; roll 2
    has a record in every cell."""
    key = (n_cells, nfeat, n_rolls)
    if key not in _rolls:
        rng = np.random.default_rng(n_cells * 7 + nfeat)
        f32 = np.float32
        x = (rng.random((n_cells, nfeat)) * (rng.random((n_cells, 1)) < .2)).astype(f32)
        x[:, 0] *= 4
        lo, up, nan = f32(.01), np.nextafter(f32(.01), f32(1)), f32('nan')
        edge = [[-0., 0., 0., 0., 0.], [0., nan, 0., 0., 0.], [1., lo, 0., 1., 0.], [2., up, .3, .2, .1], [1., nan, 0., 1., 0.],
                [3., .5, .7, .7, .2], [1.5, .6, f32(.1), f32(.1), .05], [2.5, .02, .4, .3, .9]]
        at = [0, 1, 2, 3, n_cells - 4, n_cells - 3, n_cells - 2, n_cells - 1] if n_cells >= 8 else [0]
        for c, e in zip(at, edge if n_cells >= 8 else [edge[3]]):
            x[c] = np.asarray(e, dtype=f32)[:nfeat]
        full = (rng.random((n_cells, nfeat)) + .2).astype(f32)
        _rolls[key] = [x, np.zeros((n_cells, nfeat), f32), full][:n_rolls]
    return _rolls[key]


def records_of(x, mode):
    """(cells int32, feats float32 (n, nfeat)) of a host roll: the numpy statement of the two record predicates."""
    if mode == NONZERO:
        idx = np.flatnonzero(x.view(np.uint32).any(axis=1))
        return idx.astype(np.int32), x[idx]
    f32 = np.float32
    hard = x.copy()
    with np.errstate(invalid='ignore'):
        on = x[:, 1] > f32(.01)                                  # a NaN velocity is off
        hard[:, 1] = np.where(on, x[:, 1], f32(0.))
        if x.shape[1] > 2:
            top = np.fmax(x[:, 2], np.fmax(x[:, 3], x[:, 4]))[:, None]
            hard[:, 2:] = ((x[:, 2:] == top) & (x[:, 2:] > f32(.1))).astype(f32)
    if not np.isnan(x).any():                                    # where the oracle is defined, it says the same
        assert np.array_equal(so.hard_output(torch.from_numpy(x.copy())).numpy().view(np.uint32), hard.view(np.uint32))
    idx = np.flatnonzero(on)
    return idx.astype(np.int32), hard[idx]


_single = {}


def single_roll(native, device, x, mode, capacity, key):
    """mst_roll_count / mst_roll_compact on a contiguous copy of the roll, into sentinel-filled destinations of `capacity`
    records: (ws, cells words, feats words)."""
    key = (native.path, str(device), mode, capacity) + key
    if key not in _single:
        n_cells, nfeat = x.shape
        dx = torch.from_numpy(x).to(device)
        ws = torch.full((native.roll_slices(n_cells) + 1,), -7, dtype=torch.int32, device=device)
        native.roll_count(dx, n_cells, nfeat, mode, ws, stream(device))
        cells, feats = torch.full((capacity + 1,), -7, dtype=torch.int32, device=device), poisoned((capacity + 1) * nfeat, device)
        native.roll_compact(dx, n_cells, nfeat, mode, ws, capacity, cells, feats, stream(device))
        _single[key] = (ws.cpu().numpy(), cells.cpu().numpy()[:capacity], words(feats)[:capacity * nfeat])
    return _single[key]


def rolls_check(native, device, n_cells, nfeat, mode, n_rolls, gap, lead, guard=8):
    rolls = roll_set(n_cells, nfeat, n_rolls)
    stride = n_cells * nfeat + gap
    SL = native.roll_slices(n_cells)
    host = np.full(guard + lead + n_rolls * stride + guard, POISON, dtype=np.uint32)       # the gaps hold the poison
    for k, x in enumerate(rolls):
        at = guard + lead + k * stride
        host[at:at + n_cells * nfeat] = x.view(np.uint32).reshape(-1)
    buf = torch.from_numpy(host.view(np.int32).copy()).to(device)
    assert buf.data_ptr() % 16 == 0
    xp = buf.data_ptr() + 4 * (guard + lead)
    want = [records_of(x, mode) for x in rolls]
    totals = [len(c) for c, _ in want]
    ws = torch.full((guard + n_rolls * (SL + 1) + guard,), -7, dtype=torch.int32, device=device)
    native.rolls_count(xp, stride, n_rolls, n_cells, nfeat, mode, ws.data_ptr() + 4 * guard, stream(device))
    got_ws = ws.cpu().numpy()
    assert (got_ws[:guard] == -7).all() and (got_ws[-guard:] == -7).all()
    got_ws = got_ws[guard:-guard].reshape(n_rolls, SL + 1)
    for k, x in enumerate(rolls):
        per_slice = np.bincount(want[k][0] // S, minlength=SL)
        assert got_ws[k].tolist() == [0] + np.cumsum(per_slice).tolist(), (k, got_ws[k])
    for capacity in sorted({max(totals), max(max(totals) - 1, 0), 0}):
        cells = torch.full((guard + n_rolls * capacity + guard,), -7, dtype=torch.int32, device=device)
        feats = poisoned((guard + n_rolls * capacity + guard) * nfeat, device)
        counts = torch.full((guard + n_rolls + guard,), -7, dtype=torch.int32, device=device)
        native.rolls_compact(xp, stride, n_rolls, n_cells, nfeat, mode, ws.data_ptr() + 4 * guard, capacity, cells.data_ptr() + 4 * guard,
                             feats.data_ptr() + 4 * guard * nfeat, counts.data_ptr() + 4 * guard, stream(device))
        got_c, got_f, got_n = cells.cpu().numpy(), words(feats), counts.cpu().numpy()
        assert got_n.tolist() == [-7] * guard + totals + [-7] * guard              # the TRUE totals, whatever the capacity
        assert (got_c[:guard] == -7).all() and (got_c[len(got_c) - guard:] == -7).all()
        assert (got_f[:guard * nfeat] == POISON).all() and (got_f[len(got_f) - guard * nfeat:] == POISON).all()
        got_c = got_c[guard:len(got_c) - guard].reshape(n_rolls, capacity)
        got_f = got_f[guard * nfeat:len(got_f) - guard * nfeat].reshape(n_rolls, capacity * nfeat)
        for k, x in enumerate(rolls):
            keep = min(totals[k], capacity)
            assert got_c[k, :keep].tolist() == want[k][0][:keep].tolist() and (got_c[k, keep:] == -7).all(), (k, capacity)
            assert np.array_equal(got_f[k, :keep * nfeat], want[k][1][:keep].view(np.uint32).reshape(-1)), (k, capacity)
            assert (got_f[k, keep * nfeat:] == POISON).all(), (k, capacity)     # poison sits behind the records
            one_ws, one_c, one_f = single_roll(native, device, x, mode, capacity, (n_cells, nfeat, n_rolls, k))
            assert np.array_equal(got_ws[k], one_ws) and np.array_equal(got_c[k], one_c) and np.array_equal(got_f[k], one_f), (k, capacity)
        if mode == NONZERO and capacity == max(totals) and capacity > 0:
            # the record layout is mst_clip_scatter's: it gives the rolls back bit for bit
            back = poisoned(n_rolls * n_cells * nfeat, device)
            native.clip_scatter(cells.data_ptr() + 4 * guard, feats.data_ptr() + 4 * guard * nfeat, counts.data_ptr() + 4 * guard, back,
                                n_cells, nfeat, n_clips=n_rolls, capacity=capacity, stream=stream(device))
            assert np.array_equal(words(back), np.concatenate([x.view(np.uint32).reshape(-1) for x in rolls]))
    assert np.array_equal(words(buf), host), 'x is read only'
    return totals


def _case_rolls(nfeat, mode):
    def case(native, device):
        assert native.roll_slices(S) == 1 and native.roll_slices(S + 1) == 2, 'S above is not the kernels\' slice'
        phases = set()
        for n_cells in (1, 1023, 1024, 1025, 2049):
            for n_rolls in (1, 3):
                for gap in (0, 1, 3):
                    for lead in (0, 1):
                        totals = rolls_check(native, device, n_cells, nfeat, mode, n_rolls, gap, lead)
                        phases |= {(lead + k * (n_cells * nfeat + gap)) % 4 for k in range(n_rolls)}
                if n_rolls == 3:
                    assert totals[1] == 0 and totals[2] == n_cells and (n_cells < 8 or 0 < totals[0] < n_cells)
        assert phases == {0, 1, 2, 3}                           # the rolls started at all four 16-byte phases
    case.__name__ = f'case_rolls_{"pitched" if nfeat == 5 else "unpitched"}_{"hard" if mode == HARD else "nonzero"}'
    return case


def case_rolls_err_arg(native, device):
    """Every MST_ERR_ARG case of the two entry points; a refused call writes nothing."""
    x = torch.rand(3 * 1030 * 5 + 8, device=device)
    ws = torch.full((3 * 3,), -7, dtype=torch.int32, device=device)
    cells, feats = torch.full((3 * 8,), -7, dtype=torch.int32, device=device), poisoned(3 * 8 * 5, device)
    counts = torch.full((3,), -7, dtype=torch.int32, device=device)
    count, compact = native.lib.mst_rolls_count, native.lib.mst_rolls_compact

    def args(**kw):
        a = dict(x=x.data_ptr(), roll_stride=1030 * 5, n_rolls=3, n_cells=1025, nfeat=5, mode=HARD, ws=ws.data_ptr(), capacity=8,
                 cells=cells.data_ptr(), feats=feats.data_ptr(), counts=counts.data_ptr())
        a.update(kw)
        return a
    head = ('x', 'roll_stride', 'n_rolls', 'n_cells', 'nfeat', 'mode', 'ws')
    shared = [dict(x=None), dict(ws=None), dict(n_rolls=0), dict(n_rolls=-1), dict(n_cells=0), dict(n_cells=-5), dict(n_cells=2 ** 31),
              dict(n_rolls=2 ** 21, n_cells=2 ** 20, roll_stride=2 ** 23), dict(nfeat=3), dict(nfeat=0), dict(mode=2), dict(mode=-1),
              dict(roll_stride=1025 * 5 - 1), dict(roll_stride=0), dict(roll_stride=-1030 * 5), dict(x=x.data_ptr() + 2)]
    for kw in shared:
        a = args(**kw)
        assert count(*[a[k] for k in head], None) == ERR_ARG, kw
        assert compact(*[a[k] for k in head], a['capacity'], a['cells'], a['feats'], a['counts'], None) == ERR_ARG, kw
    for kw in (dict(cells=None), dict(feats=None), dict(counts=None), dict(capacity=-1)):
        a = args(**kw)
        assert compact(*[a[k] for k in head], a['capacity'], a['cells'], a['feats'], a['counts'], None) == ERR_ARG, kw
    for t in (ws, cells, counts):
        assert (t.cpu() == -7).all()                                            # nothing was launched
    assert (words(feats) == POISON).all()
    a = args()
    assert count(*[a[k] for k in head], stream(device)) == 0
    assert compact(*[a[k] for k in head], 0, a['cells'], a['feats'], a['counts'], stream(device)) == 0       # capacity 0 is allowed
    assert (cells.cpu() == -7).all() and (counts.cpu() > 8).all() and counts.cpu().tolist() == ws.cpu().view(3, 3)[:, 2].tolist()


# ---- mst_style_sums
W = nat.STYLE_SUM_WORDS


def style_values(rows, stride, length, seed):
    """`rows` runs of `length` floats, `stride` apart: signed fractions times 1e-3, 1 or 1e3, so that every addition rounds."""
    rng = np.random.default_rng(seed)
    n = (rows - 1) * stride + length
    return ((rng.random(n) - .5) * 10. ** rng.choice([-3, 0, 3], n)).astype(np.float32)


def dot(x, y):
    """The left-to-right float64 sum of the products: a Python loop of np.float64 additions."""
    total = np.float64(0.)
    for p, q in zip(x.astype(np.float64), y.astype(np.float64)):
        total = total + p * q                 # (the product of two widened floats is exact)
    return total


def style_sums(a, a_stride, b, b_rows, b_stride, idx, K, length):
    """The host statement of mst_style_sums: K x 8 float64."""
    out = np.zeros((K, W), dtype=np.float64)
    nan = np.float64('nan')
    for k in range(K):
        row = k if idx is None else idx[k]
        x = a[k * a_stride:k * a_stride + length]
        y = b[row * b_stride:row * b_stride + length] if 0 <= row < b_rows else None
        z = b[k * b_stride:k * b_stride + length] if k < b_rows else None
        pairs = ((x, x), (y, y), (z, z), (x, y), (x, z), (y, z))
        out[k, :6] = [nan if p is None or q is None else dot(p, q) for p, q in pairs]
        out[k, 6] = length
    return out


def sums_check(native, device, idx, K, length, b_rows=6, guard=4, buffer_rows=None, a_lead=0):
    a_stride, b_stride = odd(length + 2), odd(length + 6)
    a = style_values(K, a_stride, length + a_lead, seed=length)[a_lead:]
    b = style_values(b_rows if buffer_rows is None else buffer_rows, b_stride, length, seed=length + 1)
    da = torch.from_numpy(np.concatenate([np.zeros(4 - a_lead, np.float32), a])).to(device)      # a at float offset -a_lead mod 4
    db = torch.from_numpy(b).to(device)
    buf = torch.full((K * W + 2 * guard,), float('nan'), dtype=torch.float64, device=device)
    buf.view(torch.int64)[:] = 0x7ff8000000000abc                                  # a NaN the kernel does not write
    before = buf.cpu().clone()
    didx = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=device)
    native.style_sums(da.data_ptr() + 4 * (4 - a_lead), a_stride, db, b_rows, b_stride, didx, K, length, buf.data_ptr() + 8 * guard,
                      stream(device))
    after = buf.cpu()
    assert ec.same_bits(after[:guard], before[:guard]) and ec.same_bits(after[-guard:], before[-guard:]), 'a store outside out'
    got = after[guard:-guard].numpy().reshape(K, W)
    want = style_sums(a, a_stride, b, b_rows, b_stride, idx, K, length)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (K, length, got, want)
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64)), (K, length, np.argwhere(got != want)[:8])
    assert ec.same_bits(da.cpu()[4 - a_lead:], torch.from_numpy(a)) and ec.same_bits(db.cpu(), torch.from_numpy(b))
    return got


def case_sums(native, device):
    """Every length around the lane count, one LDS stretch and past it; donors with repeats and self."""
    for length in (1, 63, 64, 65, 256, 1920):
        for K, idx in ((1, [0]), (1, [3]), (5, [2, 0, 2, 3, 5])):
            got = sums_check(native, device, idx, K, length, a_lead=length % 4)
            assert np.isfinite(got).all() and (got[:, :3] > 0).all() and (got[:, 6] == length).all() and (got[:, 7] == 0).all()
        sums_check(native, device, None, 5, length)
    got = sums_check(native, device, None, 2, 1030)              # the identity: y is z, so four of the six words coincide
    assert np.array_equal(got[:, 1], got[:, 2]) and np.array_equal(got[:, 3], got[:, 4]) and np.array_equal(got[:, 1], got[:, 5])


def case_sums_rows_outside(native, device):
    """A donor outside [0, b_rows) makes words 1, 3 and 5 NaN, a clip k >= b_rows words 2, 4 and 5; the rest stays right."""
    for idx in ([1, 6, 0], [-1, 2, -2 ** 31, 2 ** 31 - 1]):
        got = sums_check(native, device, idx, len(idx), 65)
        for k, row in enumerate(idx):
            assert np.isnan(got[k]).tolist() == ([False, True, False, True, False, True, False, False] if not 0 <= row < 6 else [False] * 8)
    got = sums_check(native, device, [2, 0, 1, 3, 0], 5, 65, b_rows=3, buffer_rows=6)
    assert np.isnan(got).tolist() == [[False] * 8] * 3 + [[False, True, True, True, True, True, False, False],
                                                          [False, False, True, False, True, True, False, False]]


def case_sums_err_arg(native, device):
    a, b = torch.rand(5 * 71, device=device), torch.rand(6 * 71, device=device)
    idx = torch.tensor([1, 0, 4], dtype=torch.int32, device=device)
    out = torch.full((3 * W + 1,), float('nan'), dtype=torch.float64, device=device)
    call = native.lib.mst_style_sums

    def args(**kw):
        v = dict(a=a.data_ptr(), a_stride=71, b=b.data_ptr(), b_rows=6, b_stride=71, idx=idx.data_ptr(), n_clips=3, len=64,
                 out=out.data_ptr(), stream=None)
        v.update(kw)
        return tuple(v[k] for k in ('a', 'a_stride', 'b', 'b_rows', 'b_stride', 'idx', 'n_clips', 'len', 'out', 'stream'))
    bad = [args(a=None), args(b=None), args(out=None), args(n_clips=0), args(n_clips=-1), args(b_rows=0), args(b_rows=-6), args(len=0),
           args(len=-1), args(len=2 ** 31), args(a_stride=-1), args(b_stride=-71), args(a=a.data_ptr() + 2), args(b=b.data_ptr() + 1),
           args(out=out.data_ptr() + 4)]
    for v in bad:
        assert call(*v) == ERR_ARG, v
    assert torch.isnan(out.cpu()).all()                                          # nothing was launched
    assert call(*args(idx=None, a_stride=0, stream=stream(device))) == 0         # a null idx and a stride of 0 are allowed
    got = out.cpu()
    assert torch.isfinite(got[:3 * W]).all() and torch.isnan(got[3 * W:]).all()


KERNEL_CASES = [case_gather_copies, case_gather_rows_outside, case_gather_err_arg,
                _case_rolls(5, NONZERO), _case_rolls(5, HARD), _case_rolls(2, NONZERO), _case_rolls(2, HARD), case_rolls_err_arg,
                case_sums, case_sums_rows_outside, case_sums_err_arg]


# ---- the composition at the C ABI
NAMES = ('mode', 'bpm', 'instr', 'used_instruments', 'bpm_target')
SLOTS = ('style', 'instr') + ec.PRED_NAMES
PICKS = [(1, 2), (3, 1), (0, 0), (4, 1), (1, 3), (2, 0), (3, 2), (1, 0)]        # windows that start inside a song


def make_batch(K):
    from style.data import WindowBatch
    return WindowBatch(C, BARS, T, True, [s for s, _ in PICKS[:K]], [r for _, r in PICKS[:K]])


def cells_of(batch):
    return batch.C * batch.bars * batch.T * 560, batch.bars * batch.T * 470


def default_capacity(n_cells):
    return min(n_cells, max(4096, n_cells // 8))


def device_chain(native, plan, params, store, batch, donors, device, score=True):
    """The chain of StyleTransferModel.transfer_windows driven through the C ABI: crops, own inputs, extract, the style swap
    through a bank, the donors' inputs, info + apply, the batched compaction and, with `score`, the hard rolls rebuilt from the
    records, note retention, the second extract and the style sums."""
    K, R = batch.K, batch.bars
    st = stream(device)
    bucket = store.buckets[(C, T, True)]
    tab = bucket['table']
    fields = [(a, b - a, plan.slot(n)[0]) for n, (a, b) in zip(NAMES, bucket['fields'])]
    win = torch.zeros(2, K, 4, dtype=torch.int32)
    store.describe(batch, win.numpy())
    win = win.to(device)
    rows = [store.songs[s]['row'] for s in batch.songs.tolist()]
    own = torch.tensor(rows, dtype=torch.int32, device=device)
    theirs = torch.tensor([rows[d] for d in donors], dtype=torch.int32, device=device)
    idx = torch.tensor(donors, dtype=torch.int32, device=device)
    xp = torch.full((K, C, R, T, 10, 56, 5), float('nan'), device=device)
    xu = torch.full((K, 1, R, T, 10, 47, 2), float('nan'), device=device)
    ws = plan.new_ws()
    ec._poison(plan, ws, True)
    for k in range(K):
        for n in NAMES + ('style',):
            plan.view(n, ws=ws, clip=k).fill_(float('nan'))
    native.clip_window(store.pools[5].cells, store.pools[5].feats, win[0], xp, K, C, R, T * 560, 5, st)
    native.clip_window(store.pools[2].cells, store.pools[2].feats, win[1], xu, K, 1, R, T * 470, 2, st)
    native.window_inputs(tab, tab.shape[0], tab.shape[1], own, K, fields, plan.clip_stride, ws, st)
    plan.forward(nat.STAGE_EXTRACT, params, xp, xu, ws=ws)
    off, _, size = plan.slot('style')
    bank = torch.full((K, size), float('nan'), device=device)
    slots = ws.data_ptr() + 4 * off
    native.clip_gather(slots, K, plan.clip_stride, bank, size, None, K, size, st)
    native.clip_gather(bank, K, size, slots, plan.clip_stride, idx, K, size, st)
    native.window_inputs(tab, tab.shape[0], tab.shape[1], theirs, K, fields, plan.clip_stride, ws, st)
    plan.forward(nat.STAGE_INFO | nat.STAGE_APPLY, params, None, None, ws=ws)
    out = dict(ws=ws, bank=bank, xp=xp, xu=xu, records={})
    for name, nfeat, n_cells in (('pitched_pred', 5, cells_of(batch)[0]), ('unpitched_pred', 2, cells_of(batch)[1])):
        capacity = default_capacity(n_cells)
        rws = torch.full((K, native.roll_slices(n_cells) + 1), -7, dtype=torch.int32, device=device)
        cells = torch.full((K, capacity), -7, dtype=torch.int32, device=device)
        feats = torch.full((K, capacity, nfeat), float('nan'), device=device)
        counts = torch.full((K,), -7, dtype=torch.int32, device=device)
        x = ws.data_ptr() + 4 * plan.slot(name)[0]
        native.rolls_count(x, plan.clip_stride, K, n_cells, nfeat, HARD, rws, st)
        native.rolls_compact(x, plan.clip_stride, K, n_cells, nfeat, HARD, rws, capacity, cells, feats, counts, st)
        out['records'][nfeat] = (cells, feats, counts, capacity)
    if score:
        hp, hu = torch.full_like(xp, float('nan')), torch.full_like(xu, float('nan'))
        out['retention'] = torch.full((K, C + 1, 8), float('nan'), dtype=torch.float64, device=device)
        for nfeat, hard, target, groups, group_cells, at in ((5, hp, xp, K * C, R * T * 560, slice(0, C)), (2, hu, xu, K, R * T * 470, slice(C, C + 1))):
            cells, feats, counts, capacity = out['records'][nfeat]
            native.clip_scatter(cells, feats, counts, hard, groups * group_cells // K, nfeat, n_clips=K, capacity=capacity, stream=st)
            scratch = torch.zeros(native.roll_metrics_scratch_bytes(groups, group_cells) // 8, dtype=torch.float64, device=device)
            rec = torch.full((groups, 8), float('nan'), dtype=torch.float64, device=device)
            native.roll_metrics(hard, target, groups, group_cells, nfeat, scratch, rec, st)
            out['retention'][:, at] = rec.view(K, -1, 8)
        plan.forward(nat.STAGE_EXTRACT, params, hp, hu, ws=ws)
        out['style_sums'] = torch.full((K, W), float('nan'), dtype=torch.float64, device=device)
        native.style_sums(slots, plan.clip_stride, bank, K, size, idx, K, size, out['style_sums'], st)
        out.update(hard_pitched=hp, hard_unpitched=hu)
    return out


def host_reference(native, plan, params, batch, donors, device, score=True):
    """The same Plan(clips = K) driven from the host: dense clips cropped on the host, set_inputs per clip, index_select of the
    style views in torch, set_inputs per clip from the donors' songs, sparse.compact(..., 'hard') per clip; with `score` the
    hard rolls densified from those records on the host, mst_roll_metrics on them, the second extract, and the Python loop of
    float64 additions over its styles.  Returns the workspace after info + apply (a clone), the bank, the per-clip SparseRolls
    and the two scores."""
    from style.sparse import compact
    K, R = batch.K, batch.bars
    clips = [wc.songs()[s] for s in batch.songs.tolist()]
    dense = wc.cropped(batch)
    xp, xu = torch.cat([p for p, _ in dense]).to(device), torch.cat([u for _, u in dense]).to(device)
    ws = plan.new_ws()
    ec._poison(plan, ws, True)
    for k, clip in enumerate(clips):
        ec._set_clip(plan, clip, k, ws)
    plan.forward(nat.STAGE_EXTRACT, params, xp, xu, ws=ws)
    styles = [plan.view('style', ws=ws, clip=k) for k in range(K)]
    bank = torch.stack(styles).clone()
    swapped = bank.index_select(0, torch.tensor(donors, device=device))
    for k in range(K):
        styles[k].copy_(swapped[k])
        ec._set_clip(plan, clips[donors[k]], k, ws)
    plan.forward(nat.STAGE_INFO | nat.STAGE_APPLY, params, None, None, ws=ws)
    out = dict(bank=bank, xp=xp, xu=xu, rolls=[])
    for k in range(K):
        out['rolls'].append((compact(plan.view('pitched_pred', (1, C, R, T, 10, 56, 5), ws=ws, clip=k), 'hard', pin=False, native=native),
                             compact(plan.view('unpitched_pred', (1, 1, R, T, 10, 47, 2), ws=ws, clip=k), 'hard', pin=False, native=native)))
    out['ws'] = ws.clone()
    if score:
        hp = torch.from_numpy(np.concatenate([p.to_numpy() for p, _ in out['rolls']])).to(device)
        hu = torch.from_numpy(np.concatenate([u.to_numpy() for _, u in out['rolls']])).to(device)
        out['retention'] = torch.zeros(K, C + 1, 8, dtype=torch.float64, device=device)
        for nfeat, hard, target, groups, group_cells, at in ((5, hp, xp, K * C, R * T * 560, slice(0, C)), (2, hu, xu, K, R * T * 470, slice(C, C + 1))):
            scratch = torch.zeros(native.roll_metrics_scratch_bytes(groups, group_cells) // 8, dtype=torch.float64, device=device)
            rec = torch.zeros(groups, 8, dtype=torch.float64, device=device)
            native.roll_metrics(hard, target, groups, group_cells, nfeat, scratch, rec, stream(device))
            out['retention'][:, at] = rec.view(K, -1, 8)
        plan.forward(nat.STAGE_EXTRACT, params, hp, hu, ws=ws)
        again = torch.stack([plan.view('style', ws=ws, clip=k) for k in range(K)]).cpu().numpy()
        size = again.shape[1]
        out['style_sums'] = torch.from_numpy(style_sums(again.reshape(-1), size, bank.cpu().numpy().reshape(-1), K, size, donors, K, size))
        out.update(hard_pitched=hp, hard_unpitched=hu, styles_again=again)
    return out


def write_song(path, seed, bars, programs, numerator=2, tpb=96, percussion=True, bpm=100):
    """A small synthetic song written with the project's own MIDI writer (style.smf): one track per program and one for
    percussion, notes on the eighth-note grid of `bars` bars of `numerator` beats."""
    from style import smf
    rng = np.random.default_rng(seed)
    mid = smf.MidiFile(ticks_per_beat=tpb)
    mid.tracks.append([smf.MetaMessage('time_signature', 0, numerator=numerator, denominator=4),
                       smf.MetaMessage('set_tempo', 0, tempo=smf.bpm2tempo(bpm))])
    for c, program in enumerate(list(programs) + ([None] if percussion else [])):
        channel = 9 if program is None else c
        events = [] if program is None else [(0, smf.Message('program_change', 0, channel=channel, program=int(program)))]
        for slot in range(1, bars * numerator * 2):       # (a note at tick 0 would make the time signature a "change")
            for _ in range(int(rng.integers(0, 3))):
                note = int(rng.integers(40, 70)) if program is None else int(rng.integers(48, 84))
                start, length = slot * tpb // 2, int(rng.integers(1, 5)) * tpb // 2
                events.append((start, smf.Message('note_on', 0, channel=channel, note=note, velocity=int(rng.integers(30, 120)))))
                events.append((start + length, smf.Message('note_off', 0, channel=channel, note=note, velocity=0)))
        events.sort(key=lambda e: e[0])
        track, now = [], 0
        for t, m in events:
            m.time, now = t - now, t
            track.append(m)
        mid.tracks.append(track)
    mid.save(str(path))
    return str(path)


def same_records(cells, feats, count, roll):
    """Row k of the batched compaction against a host SparseRoll: the count, the cells and the feature bits."""
    return count == roll.count and cells[:count].tolist() == roll.cells.tolist() and ec.same_bits(feats[:count], roll.feats)


def case_composition(native, device, K=3, donors=DONORS, gemm_tile=None):
    store = wc.make_store(device)
    batch = make_batch(K)
    plan = nat.Plan(native, make_dims(pc.SMALL, C, BARS, T, True, clips=K), device, gemm_tile=gemm_tile)
    params = ec.eval_params(native, make_dims(pc.SMALL, C, BARS, T, True)).to(device)
    got = device_chain(native, plan, params, store, batch, donors, device)
    want = host_reference(native, plan, params, batch, donors, device)
    assert ec.same_bits(got['xp'], want['xp'].reshape(got['xp'].shape)) and ec.same_bits(got['xu'], want['xu'].reshape(got['xu'].shape))
    assert ec.same_bits(got['bank'], want['bank']) and len({bytes(words(row)) for row in want['bank']}) == K
    for k in range(K):
        assert ec.same_bits(plan.view('style', ws=want['ws'], clip=k), want['bank'][donors[k]])
        for n in NAMES + SLOTS[2:]:
            assert ec.same_bits(plan.view(n, ws=got['ws'], clip=k), plan.view(n, ws=want['ws'], clip=k)), (n, k)
            assert torch.isfinite(plan.view(n, ws=want['ws'], clip=k)).all(), (n, k)
    for nfeat, which, n_cells in ((5, 0, cells_of(batch)[0]), (2, 1, cells_of(batch)[1])):
        cells, feats, counts, capacity = got['records'][nfeat]
        cells, feats, counts = cells.cpu(), feats.cpu(), counts.cpu().tolist()
        for k in range(K):
            assert same_records(cells[k], feats[k], counts[k], want['rolls'][k][which]), (nfeat, k)
            assert 0 < counts[k] < min(n_cells, capacity), (nfeat, k, counts[k])             # neither nothing nor every cell
            assert (cells[k, counts[k]:] == -7).all() and torch.isnan(feats[k, counts[k]:]).all()
    # the score: the hard rolls are the records and nothing else, and the three results are the host statement's bits
    assert ec.same_bits(got['hard_pitched'], want['hard_pitched'].reshape(got['hard_pitched'].shape))
    assert ec.same_bits(got['hard_unpitched'], want['hard_unpitched'].reshape(got['hard_unpitched'].shape))
    assert ec.same_bits(got['retention'], want['retention'])
    assert ec.counts_not_trivial(want['retention'][:, :C].cpu().numpy()) and ec.counts_not_trivial(want['retention'][:, C].cpu().numpy())
    for k in range(K):
        assert ec.same_bits(plan.view('style', ws=got['ws'], clip=k), torch.from_numpy(want['styles_again'][k])), k
    assert ec.same_bits(got['style_sums'], want['style_sums']) and torch.isfinite(want['style_sums']).all()
    # the swap matters: under identity donors clip 0 predicts something else
    if list(donors) != list(range(K)):
        plain = host_reference(native, plan, params, batch, list(range(K)), device, score=False)
        for n in SLOTS[2:]:
            assert not ec.same_bits(plan.view(n, ws=plain['ws'], clip=0), plan.view(n, ws=want['ws'], clip=0)), n
    return plan.gemm_tile
