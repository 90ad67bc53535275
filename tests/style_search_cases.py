"""Style search cases shared by the CPU-interpreter tests and the -m gpu tests: mst_style_search.  Both builds drive the SAME C
ABI; only the library (hipsim vs hipcc/gfx950) and the device differ.

What is asserted on both builds needs no gap between neighbouring scores, so no input is ever skipped or redrawn: per query the
returned rows are distinct and rankable, every score lies within B(len) of the float64 cosine, the order is the stated one, no
rankable row left out beats the last returned one by more than 2 B, and the count and the -1 / NaN tail are right.  B(len) =
(2 len + 8) 2^-24 is derived, not measured: the fmaf chain errs by at most len u sum |q_i r_i| <= len u |q| |r|, each norm by
len u relative, halved by the root, the product and the quotient add three roundings, and |cos| <= 1 (u = 2^-24).  Inputs have
magnitudes in [2^-10, 2^10], so nothing underflows.  Where the order is known without rounding (axis vectors scaled by powers
of two) the rows are asserted exactly.  With exact = True (the interpreter) every score must also equal the float32 fmaf chain
of the header bit for bit and the rows its ranking, ties included.

Buffers are poisoned with a NaN no kernel writes and carry guards, so that "every word of rows / scores exactly once, nothing
else, inputs untouched" is checked together with the values."""
import numpy as np
import torch

import eval_window_cases as wc
import style_bank_cases as sb
import transfer_cases as tc
from style import _native as nat

ERR_ARG = -1
POISON, QNAN = wc.POISON, wc.QNAN
SLAB, MAX_K = nat.SEARCH_SLAB, nat.SEARCH_MAX_K
GUARD = 16
stream, words, poisoned, odd, i32 = wc.stream, tc.words, tc.poisoned, tc.odd, sb.i32


def bound(length):
    return (2 * length + 8) * 2. ** -24


# ---- host references
def chain(q, r):
    """The float32 fmaf chains of the header for every pair: q (Q, len), r (N, len) -> scores (Q, N) float32.  The product of two
    floats is exact in float64, so float32(float64(a) * float64(b) + float64(acc)) is the fma; then np.sqrt and / in float32."""
    q, r = np.asarray(q, dtype=np.float32), np.asarray(r, dtype=np.float32)

    def dots(a, b):
        acc = np.zeros((len(a), len(b)), dtype=np.float32)
        for i in range(a.shape[1]):
            acc = (a[:, i, None].astype(np.float64) * b[None, :, i].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        return acc

    def squares(a):
        acc = np.zeros(len(a), dtype=np.float32)
        for i in range(a.shape[1]):
            acc = (a[:, i].astype(np.float64) * a[:, i].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        return acc
    with np.errstate(all='ignore'):
        nq, nr = squares(q), squares(r)
        den = np.sqrt(nq)[:, None] * np.sqrt(nr)[None, :]
        assert den.dtype == np.float32
        return dots(q, r) / den


def cos64(q, r):
    q, r = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    with np.errstate(all='ignore'):
        return (q @ r.T) / (np.sqrt((q * q).sum(1))[:, None] * np.sqrt((r * r).sum(1))[None, :])


def ranking(scores, rankable, k, order):
    """The header's order of one query's float32 scores: rows, padded with -1."""
    rows = sorted((r for r in range(len(scores)) if rankable[r]), key=lambda r: (-float(np.float32(order) * scores[r]), r))[:k]
    return rows + [-1] * (k - len(rows))


def values(rows, length, seed):
    """Signed floats with magnitudes in [2^-10, 2^10]."""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1., 1.], (rows, length)) * 2. ** rng.uniform(-10, 10, (rows, length))).astype(np.float32)


# ---- the check of a result
def check_ranking(rows, score_words, queries, bank, k, order, live=None, groups=None, exclude=None, exact=False):
    """The complete correctness condition of one result: rows (Q, k) int32 and score words (Q, k) uint32 for `queries` (Q, len)
    against `bank` (N, len), of which the first `live` rows count; (i) to (v) of the module's text, and with `exact` the bits."""
    bank, queries = np.asarray(bank, dtype=np.float32), np.asarray(queries, dtype=np.float32)
    (N, length), Q = bank.shape, len(queries)
    live = N if live is None else live
    scores = score_words.view(np.float32)
    c64 = cos64(queries, bank)
    c32 = chain(queries, bank) if exact else None
    B = bound(length)
    for q in range(Q):
        ex = -1 if (groups is None or exclude is None) else exclude[q]
        rankable = np.asarray([r < live and not (ex >= 0 and groups[r] == ex) and not np.isnan(c64[q, r]) for r in range(N)])
        n = min(k, int(rankable.sum()))
        got = rows[q].tolist()
        assert all(r >= 0 for r in got[:n]) and got[n:] == [-1] * (k - n), (q, got, n)                     # (v)
        assert (score_words[q, n:] == QNAN).all() and not np.isnan(scores[q, :n]).any(), (q, scores[q])
        assert len(set(got[:n])) == n and all(rankable[r] for r in got[:n]), (q, got)                         # (i)
        for j in range(n):
            assert abs(float(scores[q, j]) - c64[q, got[j]]) <= B, (q, j, got[j], scores[q, j], c64[q, got[j]], B)      # (ii)
        for j in range(1, n):                                                                                   # (iii)
            a, b = np.float32(order) * scores[q, j - 1], np.float32(order) * scores[q, j]
            assert a > b or (a == b and got[j - 1] < got[j]), (q, j, got, scores[q])
        if n == k:                                                                                              # (iv)
            left = rankable.copy()
            left[got] = False
            assert (order * c64[q, left] <= order * c64[q, got[-1]] + 2 * B).all(), (q, got)
        if exact:
            with np.errstate(all='ignore'):
                want = ranking(c32[q], rankable & ~np.isnan(c32[q]), k, order)
            assert got == want, (q, got, want)
            assert np.array_equal(score_words[q, :n], c32[q, got[:n]].view(np.uint32)), (q, scores[q], c32[q, got[:n]])


# ---- one checked call
def place(data, stride, lead, device):
    """(rows, len) float32 -> a device holder with row r at float `lead` + r * stride from a 16-byte boundary, the address of
    row 0, and the holder's words."""
    n, length = data.shape
    holder = torch.zeros(lead + (n - 1) * stride + length + 4, dtype=torch.float32, device=device)
    assert holder.data_ptr() % 16 == 0
    flat = np.zeros(holder.numel(), dtype=np.float32)
    for r in range(n):
        flat[lead + r * stride:lead + r * stride + length] = data[r]
    holder.copy_(torch.from_numpy(flat).to(device))
    return holder, holder.data_ptr() + 4 * lead, words(holder)


def search_check(native, device, bank, queries, k, order, n_live=None, groups=None, exclude=None, lead=0, aligned=False, bank_rows=None,
                 exact=False):
    """mst_style_search into poisoned outputs and the whole check.  `bank` (N, len) and `queries` (Q, len) float32; `aligned`: rows
    of both start on 16-byte boundaries (the 16-byte loads), else the bank starts `lead` floats off one and the strides are odd.
    bank_rows < N: the rows behind it are in memory only.  -> rows (Q, k) int32, score words (Q, k) uint32."""
    bank, queries = np.asarray(bank, dtype=np.float32), np.asarray(queries, dtype=np.float32)
    (N, length), Q = bank.shape, len(queries)
    bank_rows = N if bank_rows is None else bank_rows
    stride = (length + 3) // 4 * 4 + 4 if aligned else odd(length + 2)
    qstride = (length + 3) // 4 * 4 if aligned else odd(length + 4)
    hb, pb, kept_b = place(bank, stride, 0 if aligned else lead, device)
    hq, pq, kept_q = place(queries, qstride, 0 if aligned else (lead + 2) % 4, device)
    dlive = None if n_live is None else i32([n_live], device)
    dgroups = None if groups is None else i32(list(groups), device)
    dex = None if exclude is None else i32(list(exclude), device)
    out = poisoned(GUARD + Q * k + GUARD + Q * k + GUARD, device)
    scratch = poisoned(native.style_search_scratch_bytes(bank_rows, Q, k) // 4 + 2, device)
    p_rows, p_scores = out.data_ptr() + 4 * GUARD, out.data_ptr() + 4 * (2 * GUARD + Q * k)
    native.style_search(pb, bank_rows, stride, dlive, dgroups, pq, Q, qstride, dex, length, k, order, p_rows, p_scores, scratch, stream(device))
    after = words(out)
    assert (after != POISON).sum() == 2 * Q * k, 'every word of rows and scores is written, nothing else'
    for a in (0, GUARD + Q * k, 2 * GUARD + 2 * Q * k):
        assert (after[a:a + GUARD] == POISON).all()
    assert np.array_equal(words(hb), kept_b) and np.array_equal(words(hq), kept_q), 'the bank and the queries are read only'
    assert dgroups is None or dgroups.cpu().tolist() == list(groups)
    assert dex is None or dex.cpu().tolist() == list(exclude)
    assert (words(scratch)[-2:] == POISON).all(), 'scratch ends where mst_style_search_scratch_bytes says'
    rows = after[GUARD:GUARD + Q * k].view(np.int32).reshape(Q, k)
    score_words = after[2 * GUARD + Q * k:2 * GUARD + 2 * Q * k].reshape(Q, k)
    scores = score_words.view(np.float32)

    live = bank_rows if n_live is None else min(max(n_live, 0), bank_rows)
    check_ranking(rows, score_words, queries, bank, k, order, live, groups, exclude, exact)
    return rows, score_words


# ---- the cases
#         len  rows          queries  k   order  lead  aligned
RANDOM = [(1, 1, 1, 1, 1, 0, False),
          (1, SLAB + 1, 17, 2, -1, 1, False),
          (3, SLAB - 1, 15, 2, -1, 1, False),
          (4, SLAB, 16, MAX_K, 1, 3, False),
          (5, SLAB + 1, 17, 1, -1, 0, False),
          (63, 2 * SLAB + 3, 33, 2, 1, 1, False),
          (64, SLAB, 1, MAX_K, -1, 0, True),
          (67, SLAB + 1, 16, 2, 1, 3, False),
          (130, 2 * SLAB + 3, 33, MAX_K, -1, 0, True),
          (130, SLAB - 1, 17, 1, 1, 1, False),
          (5, 1, 33, MAX_K, 1, 0, True)]


def case_random_validity(native, device, exact=False):
    """The smallest sizes that cross every edge: lengths around the k-step (4) and the k-tile (32) and past two tiles, banks of
    one row, one slab less / exactly / more than one and three slabs, queries around a 16-query MFMA tile and past two, k = 1,
    2 and 16, both orders, banks 0, 1 and 3 floats off a 16-byte boundary with odd strides and on the 16-byte loads."""
    for n, (length, N, Q, k, order, lead, aligned) in enumerate(RANDOM):
        search_check(native, device, values(N, length, 100 + n), values(Q, length, 200 + n), k, order, lead=lead, aligned=aligned, exact=exact)


def axis_bank(axes=35, powers=(-3, 0, 5)):
    """Rows +-2^m e_j: one block of 2 * axes rows per power, so rows that tie lie 2 * axes > SLAB rows apart, in different slabs."""
    rng = np.random.default_rng(7)
    pairs = [(j, s) for j in range(axes) for s in (1, -1)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    assert 2 * axes > SLAB
    bank = np.zeros((len(powers) * len(pairs), axes), dtype=np.float32)
    for b, m in enumerate(powers):
        for i, (j, s) in enumerate(pairs):
            bank[b * len(pairs) + i, j] = s * 2. ** m
    return bank, pairs * len(powers)


def case_exact_order(native, device, exact=False):
    """Rows are axis vectors scaled by powers of two, queries have distinct small-integer components: every norm and quotient of a
    row is exact, a row's score is +-q[j] / |q| whatever its power, so the ranking is known without rounding and rows sharing
    (j, sign) tie bit for bit and come out by ascending row, from different slabs."""
    bank, pairs = axis_bank()
    axes = bank.shape[1]
    rng = np.random.default_rng(8)
    queries = np.stack([rng.permutation(axes) + 1. for _ in range(5)]) * rng.choice([-1., 1.], (5, axes))
    for order in (1, -1):
        for aligned in (False, True):
            rows, score_words = search_check(native, device, bank, queries, MAX_K, order, lead=1, aligned=aligned, exact=exact)
            for q in range(len(queries)):
                key = [order * s * int(queries[q, j]) for j, s in pairs]
                want = sorted(range(len(bank)), key=lambda r: (-key[r], r))[:MAX_K]
                assert rows[q].tolist() == want, (q, order, rows[q].tolist(), want)
                for a in range(1, MAX_K):
                    if key[want[a]] == key[want[a - 1]]:
                        assert score_words[q, a] == score_words[q, a - 1] and want[a] // SLAB != want[a - 1] // SLAB


def case_position_independence(native, device, exact=False):
    """A returned pair's score has the same bits when the bank holds that one row and the call that one query, whatever the
    alignment; duplicate rows in different slabs tie exactly and come out by ascending row."""
    length, N, Q, k = 67, 2 * SLAB + 3, 17, 4
    bank, queries = values(N, length, 31), values(Q, length, 32)
    bank[SLAB + 9] = bank[5]
    bank[2 * SLAB + 1] = bank[5]
    queries[3] = bank[5] * np.float32(.75) + values(1, length, 33)[0] * np.float32(2. ** -12)      # row 5 and its copies lead query 3
    rows, score_words = search_check(native, device, bank, queries, k, 1, lead=3, exact=exact)
    assert rows[3, :3].tolist() == [5, SLAB + 9, 2 * SLAB + 1] and len(set(score_words[3, :3].tolist())) == 1
    for q, j, aligned, lead in ((0, 0, False, 0), (3, 1, True, 0), (7, 3, False, 1), (16, 2, False, 3), (9, 0, True, 0)):
        r = int(rows[q, j])
        one_rows, one_words = search_check(native, device, bank[r:r + 1], queries[q:q + 1], 1, 1, lead=lead, aligned=aligned, exact=exact)
        assert one_rows.tolist() == [[0]] and one_words[0, 0] == score_words[q, j], (q, j, r)
    far, far_words = search_check(native, device, bank, queries, k, -1, aligned=True, exact=exact)
    q, r = 5, int(far[5, 0])
    _, one_words = search_check(native, device, bank[r:r + 1], queries[q:q + 1], 1, -1, lead=1, exact=exact)
    assert one_words[0, 0] == far_words[q, 0]


def case_rankable_edges(native, device, exact=False):
    """n_live = 0, 1, bank_rows, more and negative; own group skipped, -1 skips nothing, a group no row has, exclude without effect
    when groups are absent; zero rows, a zero query, a NaN and an inf never come back as NaN scores; k above the rankable rows."""
    length, N, Q, k = 5, SLAB + 9, 6, 3
    bank, queries = values(N, length, 41), values(Q, length, 42)
    for n_live in (0, 1, 2, SLAB, N, N + 5, 2 ** 31 - 1, -1, -2 ** 31):
        rows, _ = search_check(native, device, bank, queries, k, 1, n_live=n_live, lead=1, exact=exact)
        assert (rows >= 0).sum() == Q * min(k, max(min(n_live, N), 0))
    rows, _ = search_check(native, device, bank, queries, k, -1, n_live=N - 2, bank_rows=N - 1, aligned=True, exact=exact)
    assert rows.max() < N - 2
    groups = [r % 4 for r in range(N)]
    groups[SLAB] = -1
    exclude = [0, -1, 3, 7, -5, 1]                              # 7: a group no row has; -1 and -5 skip nothing
    for order in (1, -1):
        rows, _ = search_check(native, device, bank, queries, MAX_K, order, groups=groups, exclude=exclude, lead=3, exact=exact)
        for q in (0, 2, 5):
            assert all(groups[r] != exclude[q] for r in rows[q])
        free, _ = search_check(native, device, bank, queries, MAX_K, order, groups=groups, lead=3, exact=exact)
        assert np.array_equal(rows[[1, 3, 4]], free[[1, 3, 4]]) and not np.array_equal(rows[0], free[0])
    one = [0] * N                                               # every row in the excluded group: nothing is rankable
    rows, _ = search_check(native, device, bank, queries, 2, 1, groups=one, exclude=[0, 0, -1, 0, 0, 1], exact=exact)
    assert (rows[[0, 1, 3, 4]] == -1).all() and (rows[[2, 5]] >= 0).all()
    odd_bank = bank.copy()
    odd_bank[[0, 7, SLAB + 2]] = 0.
    odd_bank[3, 2], odd_bank[SLAB + 1, 0], odd_bank[9, 4], odd_bank[11, 1] = np.nan, np.inf, -np.inf, -0.
    odd_queries = queries.copy()
    odd_queries[2] = 0.
    odd_queries[4, 1] = np.nan
    for order in (1, -1):
        for n_live in (None, 12):                               # 12 live rows, 4 of them not rankable: k is above the rest
            rows, _ = search_check(native, device, odd_bank, odd_queries, MAX_K, order, n_live=n_live, lead=1, exact=exact)
            assert (rows[[2, 4]] == -1).all() and not np.isin(rows, [0, 7, SLAB + 2, 3, SLAB + 1, 9]).any()
            if n_live == 12:
                assert ((rows[[0, 1, 3, 5]] >= 0).sum(axis=1) == 8).all()


def case_err_arg(native, device, exact=False):
    """Every MST_ERR_ARG case of the header; a refused call writes nothing."""
    bank = torch.from_numpy(values(71, 72, 51).reshape(-1)).to(device)     # 70 rows and room behind them
    queries = torch.from_numpy(values(4, 72, 52).reshape(-1)).to(device)
    out = poisoned(64, device)
    scratch = poisoned(native.style_search_scratch_bytes(70, 3, 4) // 4 + 2, device)
    live, groups, exclude = i32([70], device), i32(list(range(70)), device), i32([1, -1, 2, 0], device)
    call = native.lib.mst_style_search
    names = ('bank', 'bank_rows', 'bank_stride', 'n_live', 'groups', 'queries', 'n_queries', 'query_stride', 'exclude', 'len', 'k', 'order',
             'rows', 'scores', 'scratch', 'stream')
    o, b, q = out.data_ptr(), bank.data_ptr(), queries.data_ptr()

    def args(**kw):
        a = dict(bank=b, bank_rows=70, bank_stride=72, n_live=live.data_ptr(), groups=groups.data_ptr(), queries=q, n_queries=3,
                 query_stride=72, exclude=exclude.data_ptr(), len=64, k=4, order=1, rows=o, scores=o + 4 * 12, scratch=scratch.data_ptr(),
                 stream=None)
        a.update(kw)
        return tuple(a[n] for n in names)
    bad = [args(bank=None), args(queries=None), args(rows=None), args(scores=None), args(scratch=None), args(bank_rows=0), args(bank_rows=-70),
           args(n_queries=0), args(n_queries=-1), args(n_queries=4097), args(len=0), args(len=-64), args(len=4097), args(k=0), args(k=-1),
           args(k=MAX_K + 1), args(order=0), args(order=2), args(order=-2), args(bank_stride=-72), args(query_stride=-1),
           args(bank=b + 2), args(queries=q + 1), args(rows=o + 2), args(scores=o + 4 * 12 + 1), args(n_live=live.data_ptr() + 2),
           args(groups=groups.data_ptr() + 1), args(exclude=exclude.data_ptr() + 2), args(scratch=scratch.data_ptr() + 4),
           # rows / scores on each other (the same words, touching in one), on the bank's rows and on the queries
           args(scores=o), args(scores=o + 4 * 11), args(rows=b), args(rows=b + 4 * (69 * 72 + 63)), args(scores=b + 4 * 72),
           args(rows=q + 4 * (2 * 72 + 63)), args(scores=q), args(bank_stride=2 ** 62), args(query_stride=2 ** 62),
           args(groups=None)]                                   # exclude without groups
    for a in bad:
        assert call(*a) == ERR_ARG, a
    assert (words(out) == POISON).all() and (words(scratch) == POISON).all()     # nothing was launched
    assert native.lib.mst_style_search_scratch_bytes(0, 3, 4) <= 0 and native.lib.mst_style_search_scratch_bytes(70, 0, 4) <= 0
    assert native.lib.mst_style_search_scratch_bytes(70, 4097, 4) <= 0 and native.lib.mst_style_search_scratch_bytes(70, 3, 0) <= 0
    assert native.lib.mst_style_search_scratch_bytes(70, 3, MAX_K + 1) <= 0 and native.lib.mst_style_search_scratch_bytes(-1, 3, 4) <= 0
    st = stream(device)
    assert call(*args(rows=b + 4 * (69 * 72 + 64), stream=st)) == 0              # disjoint by one float: allowed
    assert call(*args(scores=o + 4 * 12, stream=st)) == 0
    for ok in (args(n_live=None), args(exclude=None), args(groups=None, exclude=None), args(bank_stride=0), args(query_stride=0)):
        assert call(*ok[:-1], st) == 0, ok
    assert (words(out)[24:] == POISON).all()


def case_chain_into_mix(native, device, exact=False):
    """search -> mst_style_mix with `rows` as its idx and offsets[q] = q k equals mst_style_mix fed the same rows from the host,
    bit for bit."""
    length, N, Q, k = 67, SLAB + 5, 5, 3
    bank, queries = values(N, length, 61), values(Q, length, 62)
    stride = odd(length + 2)
    hb, pb, _ = place(bank, stride, 1, device)
    dq = torch.from_numpy(queries).to(device)
    rows = torch.full((Q, k), -7, dtype=torch.int32, device=device)
    scores = torch.zeros(Q, k, device=device)
    scratch = torch.zeros(native.style_search_scratch_bytes(N, Q, k) // 8, dtype=torch.int64, device=device)
    st = stream(device)
    offsets = i32((np.arange(Q + 1) * k).tolist(), device)
    w = torch.full((Q * k,), float(np.float32(1.) / np.float32(k)), device=device)
    mixed_dev, mixed_host = poisoned(Q * length, device), poisoned(Q * length, device)
    native.style_search(pb, N, stride, None, None, dq, Q, length, None, length, k, 1, rows, scores, scratch, st)
    native.style_mix(pb, N, stride, offsets, rows, w, Q * k, mixed_dev, length, Q, length, st)
    host_rows = rows.cpu()
    assert (host_rows >= 0).all()
    native.style_mix(pb, N, stride, offsets, i32(host_rows.reshape(-1).tolist(), device), w, Q * k, mixed_host, length, Q, length, st)
    got = words(mixed_dev)
    assert np.array_equal(got, words(mixed_host)) and (got != POISON).all()
    for q in range(Q):
        want = sb.mixed(words(hb).view(np.float32)[1:], N, stride, np.arange(Q + 1) * k, host_rows.reshape(-1).numpy(),
                        np.full(Q * k, np.float32(1.) / np.float32(k), dtype=np.float32), q, length)
        assert np.array_equal(got[q * length:(q + 1) * length], want)


KERNEL_CASES = [case_random_validity, case_exact_order, case_position_independence, case_rankable_edges, case_err_arg, case_chain_into_mix]
