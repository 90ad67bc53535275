"""Style bank cases shared by the CPU-interpreter tests and the -m gpu tests: mst_style_put, mst_style_mix and mst_info_decide.
Both builds drive the SAME C ABI; only the library (hipsim vs hipcc/gfx950) and the device differ.  Every comparison is bit
equality: a scatter is a copy, a chain of separately rounded float32 products and sums has one answer — the one a numpy loop of
np.float32 operations in the same order gives — and a total order has one ranking.  There is no tolerance to choose.

Buffers are poisoned with a NaN no kernel writes and carry guards, so that "every named float exactly once, nothing else" is
checked together with the values."""
import numpy as np
import torch

import eval_window_cases as wc
import transfer_cases as tc

ERR_ARG = -1
POISON, QNAN = wc.POISON, wc.QNAN
LENGTHS = (1, 63, 64, 65, 1025)
stream, words, poisoned, odd = wc.stream, tc.words, tc.poisoned, tc.odd


def i32(values, device):
    return torch.tensor(values, dtype=torch.int32, device=device)


# ---- mst_style_put
def put_check(native, device, rows, length, bank_rows=6, lead=0, guard=16, src_stride=None, bank_stride=None):
    """mst_style_put into a poisoned bank: `guard` floats, the bank `lead` floats further on, `guard` floats."""
    K = len(rows)
    src_stride = odd(length + 2) if src_stride is None else src_stride
    bank_stride = odd(length + 4) if bank_stride is None else bank_stride
    src = tc.source(K, src_stride, length, seed=length + K)
    dsrc = torch.from_numpy(src.view(np.int32).copy()).to(device)
    buf = poisoned(guard + lead + (bank_rows - 1) * bank_stride + length + guard, device)
    want = words(buf)
    live = 0
    for k, row in enumerate(rows):
        if 0 <= row < bank_rows:
            at = guard + lead + row * bank_stride
            want[at:at + length] = src[k * src_stride:k * src_stride + length]
            live += 1
    native.style_put(dsrc, src_stride, buf.data_ptr() + 4 * (guard + lead), bank_rows, bank_stride, i32(rows, device), K, length,
                     stream(device))
    after = words(buf)
    assert np.array_equal(after, want), (rows, length, lead, np.flatnonzero(after != want)[:8])
    assert (after != POISON).sum() == live * length             # everything named was written, nothing else was
    assert np.array_equal(words(dsrc), src), 'src is read only'


def case_put_scatters(native, device):
    """Every length around the lane count and past one workgroup's chunk, K = 1 and 5, rows out of order, banks at float
    offsets 0, 1 and 3 from a 16-byte boundary; rows back to back."""
    for length in LENGTHS:
        for rows in ([4], [3, 0, 5, 1, 2]):
            for lead in (0, 1, 3):
                put_check(native, device, rows, length, lead=lead)
    put_check(native, device, [2, 0, 3], 64, bank_stride=64, src_stride=64)


def case_put_rows_outside(native, device):
    """-1, = bank_rows and rows far outside write nothing for their clips; the other clips are written exactly once."""
    for rows in ([1, 6, 0], [-1, 2, -2 ** 31, 2 ** 31 - 1, 4], [-1], [6, 7, -5]):
        for length in (1, 65, 1025):
            put_check(native, device, rows, length, lead=1)
    put_check(native, device, [3, 1, 2, 0], 65, bank_rows=3)                 # row 3 exists in memory, not in the bank


def case_put_err_arg(native, device):
    """Every MST_ERR_ARG case; a refused call writes nothing."""
    src = torch.from_numpy(tc.source(6, 71, 64).view(np.int32).copy()).to(device)
    bank = poisoned(6 * 71, device)
    rows = i32([1, 0], device)
    call = native.lib.mst_style_put
    names = ('src', 'src_stride', 'bank', 'bank_rows', 'bank_stride', 'rows', 'n_clips', 'len', 'stream')

    def args(**kw):
        a = dict(src=src.data_ptr(), src_stride=71, bank=bank.data_ptr(), bank_rows=5, bank_stride=71, rows=rows.data_ptr(), n_clips=2,
                 len=64, stream=None)
        a.update(kw)
        return tuple(a[k] for k in names)
    b = bank.data_ptr()
    bad = [args(src=None), args(bank=None), args(rows=None), args(n_clips=0), args(n_clips=-2), args(bank_rows=0), args(bank_rows=-1),
           args(len=0), args(len=-64), args(src_stride=-1), args(bank_stride=-71), args(bank_stride=63), args(bank_stride=0),
           # the two ranges intersect: the same buffer, the source inside the bank's rows, ranges that touch in one float
           args(src=b), args(src=b + 4 * 71, bank_rows=3), args(src=b + 4 * (4 * 71 + 63)), args(bank=b + 4 * 71, src=b, bank_rows=2),
           args(src_stride=2 ** 62), args(bank_stride=2 ** 62), args(src=src.data_ptr() + 2), args(bank=b + 1), args(rows=rows.data_ptr() + 2)]
    for a in bad:
        assert call(*a) == ERR_ARG, a
    assert (words(bank) == POISON).all()                                        # nothing was launched
    assert call(*args(src=b + 4 * (71 + 64), bank_rows=2, stream=stream(device))) == 0     # disjoint by one float: allowed
    assert call(*args(bank_stride=63, bank_rows=1, stream=stream(device))) == 0            # one row has no stride
    assert call(*args(stream=stream(device))) == 0


# ---- mst_style_mix
def mix_values(rows, stride, length, seed):
    """`rows` runs of `length` floats, `stride` apart: signed fractions times 1e-3, 1 or 1e3, away from zero — every value,
    every product with a weight below and every sum of them is normal or exactly zero, so no flush mode can matter."""
    rng = np.random.default_rng(seed)
    n = (rows - 1) * stride + length
    return ((rng.random(n) + .25) * rng.choice([-1., 1.], n) * 10. ** rng.choice([-3, 0, 3], n)).astype(np.float32)


def mix_weights(n, seed):
    """Weights in +-[1/4, 2], with zeros, a negative zero, ones and negatives among them."""
    rng = np.random.default_rng(seed)
    w = ((rng.random(n) * 1.75 + .25) * rng.choice([-1., 1.], n)).astype(np.float32)
    w[rng.random(n) < .15] = 0.
    if n > 2:
        w[1], w[2] = -0., 1.
    return w


def mixed(bank, bank_rows, bank_stride, offsets, idx, w, k, length):
    """The host statement for clip k: the float32 words, or None where the device owes quiet NaNs."""
    e0, e1 = int(offsets[k]), int(offsets[k + 1])
    if e0 < 0 or e1 > len(idx) or e1 <= e0 or any(not 0 <= int(r) < bank_rows for r in idx[e0:e1]):
        return None
    row = lambda e: bank[int(idx[e]) * bank_stride:int(idx[e]) * bank_stride + length]
    acc = np.float32(w[e0]) * row(e0)                          # the first product is not added to a zero
    for e in range(e0 + 1, e1):
        acc = acc + np.float32(w[e]) * row(e)                  # two float32 ufuncs: the product is rounded before the sum
    assert acc.dtype == np.float32
    return acc.view(np.uint32)


def mix_check(native, device, offsets, idx, w, length, bank_rows=6, aligned=True, lead=0, guard=16, buffer_rows=None):
    """mst_style_mix into a poisoned buffer.  `aligned`: the bank's rows start on 16-byte boundaries (the 16-byte loads);
    otherwise the bank starts one float off and its stride is odd (the scalar loads)."""
    K = len(offsets) - 1
    bank_stride = (length + 3) // 4 * 4 + 4 if aligned else odd(length + 2)
    dst_stride = odd(length + 4)
    bank = mix_values(bank_rows if buffer_rows is None else buffer_rows, bank_stride, length, seed=length + K)
    holder = torch.zeros(len(bank) + 4, dtype=torch.float32, device=device)
    assert holder.data_ptr() % 16 == 0
    shift = 0 if aligned else 1
    holder[shift:shift + len(bank)] = torch.from_numpy(bank).to(device)
    kept = words(holder)
    buf = poisoned(guard + lead + (K - 1) * dst_stride + length + guard, device)
    want = words(buf)
    nans = 0
    for k in range(K):
        at = guard + lead + k * dst_stride
        row = mixed(bank, bank_rows, bank_stride, offsets, idx, w, k, length)
        want[at:at + length] = QNAN if row is None else row
        nans += row is None
    doff, didx = i32(offsets, device), i32(idx, device)
    dw = torch.from_numpy(np.asarray(w, dtype=np.float32)).to(device)
    native.style_mix(holder.data_ptr() + 4 * shift, bank_rows, bank_stride, doff, didx, dw, len(idx), buf.data_ptr() + 4 * (guard + lead),
                     dst_stride, K, length, stream(device))
    after = words(buf)
    assert np.array_equal(after, want), (offsets, length, aligned, lead, np.flatnonzero(after != want)[:8])
    assert (after != POISON).sum() == K * length                # everything named was written, nothing else was
    assert np.array_equal(words(holder), kept) and doff.cpu().tolist() == list(offsets) and didx.cpu().tolist() == list(idx)
    assert np.array_equal(words(dw), np.asarray(w, dtype=np.float32).view(np.uint32)), 'the bank, offsets, idx and w are read only'
    return after, nans


def entry_lists(counts, bank_rows, seed):
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(counts)]).tolist()
    idx = rng.integers(0, bank_rows, offsets[-1]).tolist()
    return offsets, idx, mix_weights(offsets[-1], seed + 1)


def case_mix_sums(native, device):
    """1, 2, 7, 200 and 300 entries per clip (300: more than one staged stretch of entries) at every length, on the 16-byte and
    on the scalar loads, destinations at float offsets 0, 1 and 3; zero and negative weights; rows repeated within a clip."""
    for length in LENGTHS:
        offsets, idx, w = entry_lists([1, 2, 7, 200, 300], 6, seed=length)
        idx[3:10] = [5, 2, 5, 5, 0, 2, 5]                                       # clip 2 names row 5 four times
        for aligned in (True, False):
            for lead in (0, 1, 3):
                _, nans = mix_check(native, device, offsets, idx, w, length, aligned=aligned, lead=lead)
                assert nans == 0
    mix_check(native, device, [0, 3], [1, 1, 1], [.5, .25, -2.], 65)             # K = 1
    mix_check(native, device, [0, 2, 2 + 257], [0, 1] + [3] * 257, mix_weights(259, 5), 64)


def case_mix_weight_one_copies(native, device):
    """One entry of weight 1 is the row's bits, whichever loads serve it."""
    for length in LENGTHS:
        for aligned in (True, False):
            idx = [4, 0, 4, 2, 5]
            after, _ = mix_check(native, device, list(range(6)), idx, [1.] * 5, length, aligned=aligned, lead=1)
            stride = (length + 3) // 4 * 4 + 4 if aligned else odd(length + 2)
            bank = mix_values(6, stride, length, seed=length + 5).view(np.uint32)
            for k, row in enumerate(idx):
                at = 16 + 1 + k * odd(length + 4)
                assert np.array_equal(after[at:at + length], bank[row * stride:row * stride + length])


def case_mix_nan_clips(native, device):
    """An empty range, decreasing offsets, offsets outside [0, n_entries] and an idx outside [0, bank_rows) each give
    0x7fc00000 in that clip only; bank_rows says where the bank ends."""
    w = mix_weights(8, 3)
    for length in (1, 65, 1025):
        for aligned in (True, False):
            _, nans = mix_check(native, device, [0, 3, 2, 5, 5], [1, 0, 2, 3, 4, 5, 0, 1], w, length, aligned=aligned)
            assert nans == 2                                    # clip 1 decreases, clip 3 is empty, clips 0 and 2 are right
            _, nans = mix_check(native, device, [-1, 2, 4, 9], [1, 0, 2, 3, 4, 5, 0, 1], w, length, aligned=aligned)
            assert nans == 2                                    # clip 0 starts before, clip 2 ends behind the entries
            for outside in (6, -1, 2 ** 31 - 1, -2 ** 31):
                _, nans = mix_check(native, device, [0, 2, 5, 8], [1, 0, 2, outside, 4, 5, 0, 1], w, length, aligned=aligned, lead=3)
                assert nans == 1
    _, nans = mix_check(native, device, [0, 2, 4], [0, 2, 3, 1], w[:4], 65, bank_rows=3, buffer_rows=6)   # row 3 is in memory only
    assert nans == 1


def case_mix_err_arg(native, device):
    bank = torch.from_numpy(mix_values(6, 72, 64, 1)).to(device)
    dst = poisoned(4 * 72, device)
    off, idx, w = i32([0, 1, 3], device), i32([1, 0, 2], device), torch.tensor([1., .5, .5], device=device)
    call = native.lib.mst_style_mix
    names = ('bank', 'bank_rows', 'bank_stride', 'offsets', 'idx', 'w', 'n_entries', 'dst', 'dst_stride', 'n_clips', 'len', 'stream')

    def args(**kw):
        a = dict(bank=bank.data_ptr(), bank_rows=6, bank_stride=72, offsets=off.data_ptr(), idx=idx.data_ptr(), w=w.data_ptr(),
                 n_entries=3, dst=dst.data_ptr(), dst_stride=72, n_clips=2, len=64, stream=None)
        a.update(kw)
        return tuple(a[k] for k in names)
    d = dst.data_ptr()
    bad = [args(bank=None), args(offsets=None), args(idx=None), args(w=None), args(dst=None), args(n_clips=0), args(n_clips=-1),
           args(bank_rows=0), args(bank_rows=-6), args(n_entries=0), args(n_entries=-3), args(len=0), args(len=-1), args(bank_stride=-72),
           args(dst_stride=-1), args(dst_stride=63), args(dst_stride=0),
           # the bank's rows and the destinations intersect: the same buffer, destinations inside the rows, touching in one float
           args(bank=d, bank_rows=2), args(bank=d, bank_rows=3, dst=d + 4 * 72, n_clips=1), args(bank=d + 4 * (72 + 63), bank_rows=1),
           args(bank_stride=2 ** 62), args(dst_stride=2 ** 62, n_clips=3),
           args(bank=bank.data_ptr() + 2), args(dst=d + 1), args(offsets=off.data_ptr() + 2), args(idx=idx.data_ptr() + 1), args(w=w.data_ptr() + 2)]
    for a in bad:
        assert call(*a) == ERR_ARG, a
    assert (words(dst) == POISON).all()                                         # nothing was launched
    assert call(*args(bank=d + 4 * (72 + 64), bank_rows=1, stream=stream(device))) == 0    # disjoint by one float: allowed
    dst.fill_(POISON)
    assert call(*args(bank_stride=0, stream=stream(device))) == 0               # a stride of 0: every row is the same run
    assert call(*args(dst_stride=63, n_clips=1, stream=stream(device))) == 0    # one clip has no stride
    assert (words(dst) != POISON).sum() == 2 * 64


# ---- mst_info_decide
N_LOGITS, N_GROUPS, ROW = 41, 11, 51
PERC = N_LOGITS - 1
STRIDE = 401                             # an odd clip stride; the six slots of a clip, out of order, gaps between them
IP, MP, BP, INSTR, MODE, BPM = 7, 397, 53, 60, 330, 57


def group_of():
    from style.data import group_of_instrument
    return list(group_of_instrument)


def ranking(x):
    """The stable descending sort with NaNs last: indices."""
    x = np.asarray(x, dtype=np.float32)
    return sorted(range(len(x)), key=lambda i: (1, 0., i) if np.isnan(x[i]) else (0, -float(x[i]), i))


def decision(x, mode, bpm, channels):
    """(picks, percussion's rank, mode index, feature rows float32 (channels, 51), rounded bpm float32) of one clip's predictions."""
    from style.data import _instrument_categories, encode_instruments
    order = ranking(x)
    picks = [i for i in order if i != PERC][:channels]
    rows = encode_instruments([_instrument_categories[i] for i in picks]).astype(np.float32)
    assert rows.shape == (channels, ROW)
    return picks, order.index(PERC), int(mode[1] > mode[0]), rows, np.float32(np.rint(np.float32(bpm)))


def pooled(x, modes, bpms, n):
    """The fp32 left-to-right sums over clips 0 .. n - 1, started from clip 0's values; bpm divided by the count."""
    x, modes, bpms = (np.asarray(a, dtype=np.float32) for a in (x, modes, bpms))
    sx, sm, sb = x[0].copy(), modes[0].copy(), np.float32(bpms[0])
    for c in range(1, n):
        sx, sm, sb = sx + x[c], sm + modes[c], np.float32(sb + bpms[c])
    return sx, sm, np.float32(sb / np.float32(n))


def decide_check(native, device, x, modes, bpms, channels, pool=False, live=None, guard=8):
    """mst_info_decide on K clips laid out STRIDE apart in a poisoned buffer; returns the decision records."""
    x, modes, bpms = np.asarray(x, dtype=np.float32), np.asarray(modes, dtype=np.float32), np.asarray(bpms, dtype=np.float32)
    K = len(x)
    host = np.full(guard + K * STRIDE + guard, POISON, dtype=np.uint32)
    for k in range(K):
        at = guard + k * STRIDE
        host[at + IP:at + IP + N_LOGITS] = x[k].view(np.uint32)
        host[at + MP:at + MP + 2] = modes[k].view(np.uint32)
        host[at + BP] = bpms[k:k + 1].view(np.uint32)[0]
    buf = torch.from_numpy(host.view(np.int32).copy()).to(device)
    rec = torch.full((guard + K * (channels + 2) + guard,), -7, dtype=torch.int32, device=device)
    dlive = None if live is None else i32([live], device)
    p = lambda off: buf.data_ptr() + 4 * (guard + off)
    native.info_decide(p(IP), p(MP), p(BP), STRIDE, N_LOGITS, group_of(), N_GROUPS, channels, K, pool, dlive, p(INSTR), p(MODE), p(BPM),
                       STRIDE, rec.data_ptr() + 4 * guard, stream(device))
    want, want_rec = host.copy(), []
    n = K if live is None else min(max(live, 1), K)
    for k in range(K):
        picks, perc, mode, rows, bpm = decision(*(pooled(x, modes, bpms, n) if pool else (x[k], modes[k], bpms[k])), channels)
        at = guard + k * STRIDE
        want[at + INSTR:at + INSTR + channels * ROW] = rows.reshape(-1).view(np.uint32)
        want[at + MODE:at + MODE + 2] = np.asarray([1 - mode, mode], dtype=np.float32).view(np.uint32)
        want[at + BPM] = np.asarray([bpm]).view(np.uint32)[0]
        want_rec.append(picks + [perc, mode])
    after, got_rec = words(buf), rec.cpu().numpy()
    assert np.array_equal(after, want), (channels, pool, live, np.flatnonzero(after != want)[:8])
    assert (got_rec[:guard] == -7).all() and (got_rec[-guard:] == -7).all()
    got_rec = got_rec[guard:-guard].reshape(K, channels + 2)
    assert got_rec.tolist() == want_rec, (got_rec.tolist(), want_rec)
    return got_rec


def logits(K, seed):
    rng = np.random.default_rng(seed)
    x = rng.permutation(K * N_LOGITS).reshape(K, N_LOGITS).astype(np.float32) / 8 - 17       # distinct, signed, exact in fp32
    return x, rng.standard_normal((K, 2)).astype(np.float32), (rng.random(K) * 120 + 40).astype(np.float32)


def case_decide_picks(native, device):
    """Distinct logits at C = 1, 2 and 5: the picks are the first C non-percussion entries of the stable descending sort, and
    what style_transfer.select_instruments(x, C + 1) picks — all of it when percussion is within the top C + 1, else its first
    C; percussion first, last and in the middle of the ranking."""
    from style.data import _instrument_categories
    from style.style_transfer import select_instruments
    for channels in (1, 2, 5):
        x, modes, bpms = logits(6, seed=channels)
        x[0, PERC], x[1, PERC], x[2, PERC] = 1000., -1000., -1000.
        x[2, PERC] = np.sort(x[2])[-2] + .0625                  # percussion first, last, and second: between the top two pitched
        rec = decide_check(native, device, x, modes, bpms, channels)
        assert rec[0, channels] == 0 and rec[1, channels] == PERC and rec[2, channels] == 1
        inside = 0
        for k in range(len(x)):
            programs, unpitched = select_instruments(x[k], channels + 1)
            theirs = [_instrument_categories.index(p) for p in programs]
            assert unpitched == (rec[k, channels] <= channels)
            assert rec[k, :channels].tolist() == (theirs if unpitched else theirs[:channels]), k
            inside += unpitched
        assert 0 < inside < len(x)
    decide_check(native, device, *logits(1, seed=9), 5)                         # K = 1


def case_decide_ties_and_nans(native, device):
    """Ties go to the lower index, percussion's ties included; a NaN ranks after every number, NaNs among themselves by index;
    all logits equal; all NaN."""
    for channels in (1, 2, 5):
        x, modes, bpms = logits(7, seed=10 + channels)
        top = x.max() + 1
        x[0, [30, 3, 17]] = top                                 # a three-way tie at the top: 3, 17, 30
        x[1, [PERC, 5]] = top                                   # percussion ties with a lower index: 5 comes first
        x[2, [0, 39]] = np.nan
        x[2, 20] = -np.inf
        x[3, :] = 2.5
        x[4, :] = np.nan
        x[5, :PERC - 1] = np.nan                                # one number among the pitched: it is the first pick
        x[5, PERC - 1:] = [5., 1.]
        x[6, [2, 9]] = [0., -0.]                                # the two zeros are equal
        x[6, [4, 6]] = x[6].min() - 1
        rec = decide_check(native, device, x, modes, bpms, channels)
        assert rec[0, :min(channels, 3)].tolist() == [3, 17, 30][:channels] and rec[1, 0] == 5 and rec[1, channels] == 1
        assert rec[3, :channels].tolist() == list(range(channels)) and rec[3, channels] == PERC
        assert rec[4, :channels].tolist() == list(range(channels)) and rec[4, channels] == PERC
        assert rec[5, 0] == PERC - 1 and rec[5, channels] == 1
        assert ranking(x[2])[-2:] == [0, 39] and ranking(x[2])[-3] == 20


def case_decide_mode_and_bpm(native, device):
    """The mode one-hot: the larger logit, index 0 when they are equal (zeros of either sign included); bpm: halves go to even."""
    x, _, _ = logits(8, seed=20)
    modes = [[2., 1.], [1., 2.], [.5, .5], [-3., -3.], [0., -0.], [-0., 0.], [-1., -2.], [-2., -1.]]
    bpms = [99.5, 100.5, 101.5, 120.49, 120.51, .5, 1.5, 87.]
    rec = decide_check(native, device, x, modes, bpms, 2)
    assert rec[:, 3].tolist() == [0, 1, 0, 0, 0, 0, 0, 1]
    assert np.rint(np.asarray(bpms, dtype=np.float32)).tolist() == [100., 100., 102., 120., 121., 0., 2., 87.]


def case_decide_pooled(native, device):
    """Pooled: the per-clip decision on the fp32 left-to-right sums over the first `live` clips, written to every clip; live = 1,
    K - 1, K, NULL, and values outside [1, K], which are clamped."""
    K = 5
    for channels in (1, 2, 5):
        rng = np.random.default_rng(30 + channels)
        x = (rng.standard_normal((K, N_LOGITS)) * 10. ** rng.integers(-2, 3, (K, N_LOGITS))).astype(np.float32)     # every sum rounds
        modes = rng.standard_normal((K, 2)).astype(np.float32)
        bpms = (rng.random(K) * 120 + 40).astype(np.float32)
        seen = set()
        for live in (1, K - 1, K, None, 0, K + 3, -2):
            rec = decide_check(native, device, x, modes, bpms, channels, pool=True, live=live)
            assert (rec == rec[0]).all()
            seen.add(tuple(rec[0].tolist()))
        assert len(seen) > 1                                    # the live count matters
    x, modes, bpms = logits(3, seed=40)
    x[1, 7] = np.nan                                            # a NaN of a counted clip reaches the sum: 7 ranks last
    rec = decide_check(native, device, x, modes, [100., 101., 102.5], 2, pool=True, live=2)
    assert 7 not in rec[0, :2].tolist()
    decide_check(native, device, x, modes, [100., 101., 102.5], 2, pool=True, live=1)


def case_decide_err_arg(native, device):
    buf = poisoned(3 * STRIDE, device)
    rec = torch.full((3 * 4,), -7, dtype=torch.int32, device=device)
    live = i32([2], device)
    call = native.lib.mst_info_decide
    groups = (nat_c().c_int32 * (N_LOGITS - 1))(*group_of())
    names = ('ip', 'mp', 'bp', 'pred_stride', 'n_logits', 'group_of', 'n_groups', 'channels', 'n_clips', 'pool', 'live', 'instr', 'mode',
             'bpm', 'out_stride', 'decisions', 'stream')
    p = lambda off: buf.data_ptr() + 4 * off

    def args(**kw):
        a = dict(ip=p(IP), mp=p(MP), bp=p(BP), pred_stride=STRIDE, n_logits=N_LOGITS, group_of=groups, n_groups=N_GROUPS, channels=2,
                 n_clips=3, pool=0, live=live.data_ptr(), instr=p(INSTR), mode=p(MODE), bpm=p(BPM), out_stride=STRIDE,
                 decisions=rec.data_ptr(), stream=None)
        a.update(kw)
        return tuple(a[k] for k in names)
    wrong = (nat_c().c_int32 * (N_LOGITS - 1))(*group_of())
    wrong[7] = N_GROUPS
    negative = (nat_c().c_int32 * (N_LOGITS - 1))(*group_of())
    negative[0] = -1
    bad = [args(ip=None), args(mp=None), args(bp=None), args(group_of=None), args(instr=None), args(mode=None), args(bpm=None),
           args(decisions=None), args(n_clips=0), args(n_clips=-1), args(n_logits=1), args(n_logits=0), args(n_logits=65), args(n_groups=0),
           args(n_groups=128), args(channels=0), args(channels=-1), args(channels=N_LOGITS), args(pred_stride=-1), args(out_stride=-STRIDE),
           args(out_stride=2 * ROW - 1), args(group_of=wrong), args(group_of=negative),
           # a clip's results on its predictions or on one another
           args(instr=p(IP)), args(instr=p(IP - 2 * ROW + 1)), args(mode=p(MP + 1)), args(bpm=p(BP)), args(mode=p(INSTR + 2 * ROW - 1)),
           args(bpm=p(MODE + 1)), args(bpm=p(IP + N_LOGITS - 1)),
           args(ip=p(IP) + 2), args(mp=p(MP) + 1), args(bp=p(BP) + 2), args(instr=p(INSTR) + 2), args(mode=p(MODE) + 1), args(bpm=p(BPM) + 2),
           args(decisions=rec.data_ptr() + 2), args(live=live.data_ptr() + 1)]
    for a in bad:
        assert call(*a) == ERR_ARG, a
    assert (words(buf) == POISON).all() and (rec.cpu() == -7).all()              # nothing was launched
    buf[:] = 0
    buf.view(torch.float32)[:] = torch.arange(3 * STRIDE, dtype=torch.float32, device=device) % 37
    assert call(*args(live=None, pool=1, stream=stream(device))) == 0           # a null `live` is allowed: all clips
    assert call(*args(stream=stream(device))) == 0
    assert (rec.cpu() >= 0).all()


def nat_c():
    from style import _native as nat
    return nat.C


# ---- the composition at the C ABI
def case_chain(native, device, K=3, gemm_tile=None):
    """crops -> mst_window_inputs -> extract -> mst_style_put (one clip dropped by -1) -> mst_style_mix (a stored row, a blend,
    a row named twice) -> info -> mst_info_decide -> apply on a Plan(clips = K) at SMALL widths, against the same plan driven
    from the host: host-cropped clips, set_inputs per clip, the numpy mix written into the style slots and `decision` taken on
    the downloaded predictions.  Every slot the chain writes is identical in every bit, per clip and pooled."""
    import eval_cases as ec
    import parity_cases as pc
    from simutil import make_dims
    from style import _native as nat
    C, T, BARS = wc.C, wc.T, wc.BARS
    store = wc.make_store(device)
    batch = tc.make_batch(K)
    plan = nat.Plan(native, make_dims(pc.SMALL, C, BARS, T, True, clips=K), device, gemm_tile=gemm_tile)
    params = ec.eval_params(native, make_dims(pc.SMALL, C, BARS, T, True)).to(device)
    st = stream(device)
    off, _, size = plan.slot('style')
    slot = lambda ws, name: ws.data_ptr() + 4 * plan.slot(name)[0]
    rows = [2, -1, 0] + list(range(3, K))                       # clip 1 is dropped: a padded batch's repeat
    styles = [[(0, np.float32(1.))], [(2, np.float32(.5)), (0, np.float32(-.25)), (2, np.float32(.125))], [(2, np.float32(1.))]]
    styles += [[(0, np.float32(1.) / np.float32(3)), (2, np.float32(2.) / np.float32(3))] for _ in range(K - 3)]
    offsets = np.concatenate([[0], np.cumsum([len(e) for e in styles])]).astype(np.int32)
    idx = np.asarray([r for e in styles for r, _ in e], dtype=np.int32)
    w = np.asarray([x for e in styles for _, x in e], dtype=np.float32)
    out = {}
    for pool in (False, True):
        # the device path
        bucket = store.buckets[(C, T, True)]
        tab = bucket['table']
        fields = [(a, b - a, plan.slot(n)[0]) for n, (a, b) in zip(tc.NAMES, bucket['fields'])]
        win = torch.zeros(2, K, 4, dtype=torch.int32)
        store.describe(batch, win.numpy())
        win = win.to(device)
        own = i32([store.songs[s]['row'] for s in batch.songs.tolist()], device)
        xp = torch.full((K, C, BARS, T, 10, 56, 5), float('nan'), device=device)
        xu = torch.full((K, 1, BARS, T, 10, 47, 2), float('nan'), device=device)
        ws = plan.new_ws()
        ec._poison(plan, ws, True)
        native.clip_window(store.pools[5].cells, store.pools[5].feats, win[0], xp, K, C, BARS, T * 560, 5, st)
        native.clip_window(store.pools[2].cells, store.pools[2].feats, win[1], xu, K, 1, BARS, T * 470, 2, st)
        native.window_inputs(tab, tab.shape[0], tab.shape[1], own, K, fields, plan.clip_stride, ws, st)
        plan.forward(nat.STAGE_EXTRACT, params, xp, xu, ws=ws)
        bank = torch.full((K + 1, size), float('nan'), device=device)
        native.style_put(slot(ws, 'style'), plan.clip_stride, bank, K, size, i32(rows, device), K, size, st)
        native.style_mix(bank, K, size, i32(offsets, device), i32(idx, device), torch.from_numpy(w).to(device), len(idx), slot(ws, 'style'),
                         plan.clip_stride, K, size, st)
        plan.forward(nat.STAGE_INFO, params, None, None, ws=ws)
        rec = torch.full((K, C + 2), -7, dtype=torch.int32, device=device)
        live = i32([K - 1], device)
        native.info_decide(slot(ws, 'instruments_pred'), slot(ws, 'mode_pred'), slot(ws, 'bpm_pred'), plan.clip_stride, N_LOGITS, group_of(),
                           N_GROUPS, C, K, pool, live, slot(ws, 'instr'), slot(ws, 'mode'), slot(ws, 'bpm'), plan.clip_stride, rec, st)
        plan.forward(nat.STAGE_APPLY, params, None, None, ws=ws)
        # the host path: the same plan, dense clips cropped on the host, set_inputs per clip
        clips = [wc.songs()[s] for s in batch.songs.tolist()]
        dense = wc.cropped(batch)
        hp, hu = torch.cat([p for p, _ in dense]).to(device), torch.cat([u for _, u in dense]).to(device)
        ws2 = plan.new_ws()
        ec._poison(plan, ws2, True)
        for k, clip in enumerate(clips):
            ec._set_clip(plan, clip, k, ws2)
        plan.forward(nat.STAGE_EXTRACT, params, hp, hu, ws=ws2)
        own_styles = torch.stack([plan.view('style', ws=ws2, clip=k) for k in range(K)]).cpu()
        want_bank = np.full((K + 1, size), np.nan, dtype=np.float32)
        for k, row in enumerate(rows):
            if row >= 0:
                want_bank[row] = own_styles[k].numpy()
        assert np.array_equal(np.isnan(want_bank).all(axis=1), [False, True, False] + [False] * (K - 3) + [True])
        got_bank = bank.cpu().numpy()
        live_rows = ~np.isnan(want_bank).all(axis=1)
        assert np.array_equal(got_bank[live_rows].view(np.uint32), want_bank[live_rows].view(np.uint32)) and np.isnan(got_bank[~live_rows]).all()
        for k in range(K):
            mix = mixed(want_bank.reshape(-1), K, size, offsets, idx, w, k, size).view(np.float32)
            plan.view('style', ws=ws2, clip=k).copy_(torch.from_numpy(mix.copy()))
        plan.forward(nat.STAGE_INFO, params, None, None, ws=ws2)
        pred = [[plan.view(n, ws=ws2, clip=k).cpu().numpy().reshape(-1) for n in ('instruments_pred', 'mode_pred', 'bpm_pred')] for k in range(K)]
        one = pooled([p[0] for p in pred], [p[1] for p in pred], [p[2][0] for p in pred], K - 1) if pool else None
        want_rec = []
        for k in range(K):
            picks, perc, mode, feats, bpm = decision(*(one if pool else (pred[k][0], pred[k][1], pred[k][2][0])), C)
            plan.view('instr', ws=ws2, clip=k).copy_(torch.from_numpy(feats.reshape(-1)))
            plan.view('mode', ws=ws2, clip=k).copy_(torch.tensor([1. - mode, float(mode)]))
            plan.view('bpm', ws=ws2, clip=k).copy_(torch.tensor([float(bpm)]))
            want_rec.append(picks + [perc, mode])
        plan.forward(nat.STAGE_APPLY, params, None, None, ws=ws2)
        assert rec.cpu().tolist() == want_rec
        for k in range(K):
            for n in tc.NAMES + tc.SLOTS:
                a, b = plan.view(n, ws=ws, clip=k), plan.view(n, ws=ws2, clip=k)
                assert ec.same_bits(a, b) and torch.isfinite(b).all(), (n, k, pool)
        assert ec.same_bits(plan.view('style', ws=ws, clip=0), own_styles[2].to(device))      # one entry of weight 1: the row's bits
        out[pool] = want_rec
    assert all(r == out[True][0] for r in out[True])
    return plan.gemm_tile


KERNEL_CASES = [case_put_scatters, case_put_rows_outside, case_put_err_arg,
                case_mix_sums, case_mix_weight_one_copies, case_mix_nan_clips, case_mix_err_arg,
                case_decide_picks, case_decide_ties_and_nans, case_decide_mode_and_bpm, case_decide_pooled, case_decide_err_arg]
