#!/usr/bin/env python3
"""Developer tool: the rate of training on windows of resident songs.  A synthetic style.data.SongStore (tools/synth.py: C = 4,
T = 4, songs of 24 to 64 bars, with percussion) feeds the loop `store.sample` -> StyleTransferModel.train_windows ->
FusedAdam.step at R = 16 bars; printed are clip-iterations per second for K = 8 and K = 64 clips per batch (host clock around
a window that ends in a device synchronise, after a warm-up that includes the hipGraph capture; the median of --runs windows
and their spread).
  --one-clip   also times style.train.train(fused=True, sparse_input=True) — the one-clip loop — on the same songs cut to 16
               bars, in iterations (= clips) per second;
  --kernels    also times, under device events, the two mst_clip_window launches that crop 64 clips against mst_clip_scatter
               writing the same destinations from per-clip record buffers (both are bound by the same stores).
  --eval       times held-out evaluation instead of training: style.train.evaluate_windows rounds over the store's fixed
               windows (windows per second, for every K of --clips; --eval-stride sets the windows' stride), beside it
               style.train.evaluate on the same songs, one song per call (songs per second), and, under device events, the
               two launches a windowed round adds: mst_window_inputs and mst_eval_accumulate at 64 clips.
  --transfer   times batched style transfer instead of training: StyleTransferModel.transfer_windows for every K of --clips,
               with and without score (windows per second, --iters windows per timed stretch), interleaved with the per-window
               Python surface doing the same work (extract_style, predict_song_info, apply_style, hard_output_sparse), and,
               under device events, the calls it adds at 64 clips: mst_clip_gather, mst_rolls_count, mst_rolls_compact and
               mst_style_sums.  The model's velocity biases are moved first so that 2 % of the cells are notes.
  --styles     times the style bank instead of training: StyleTransferModel.encode_styles over the store (windows per second)
               and transfer_styles — every clip a blend of two songs' means, instruments 'each' — for every K of --clips,
               interleaved with transfer_windows at the same K on the same windows (the path without the bank: the three new
               launches are the difference) and with the per-window Python surface with select_instruments on the host in the
               loop; and, under device events, mst_style_put, mst_style_mix and mst_info_decide at 64 clips.
  --rotate     times the rotating store instead: the loop sample -> train_windows -> step on a ring SongStore(resident=--songs)
               that admits M pre-sparsified songs after every E-th iteration, (E, M) = (16, 4) and (4, 4), for every K of
               --clips, alternating in one process with the same loop without refresh (the yardstick: train_windows as it
               was, on the same store, so that one captured graph serves both legs); reported are both rates, their ratio and the host time of `admit` on the loop thread; and, under
               device events, one refresh of four songs: the mst_store_admit launch against the 5 x 4 separate copies `add`
               makes for the same songs and against a device-to-device copy of the same bytes.
  --search     times style search alone (no songs, no model): mst_style_search of Q = 64 queries against N = 4 096 and 65 536
               rows of D = 256 floats, k = 8, under device events — the call, and its two launches apart (kernel durations
               from torch.profiler; null where the profiler reports none) — beside a device-to-device copy of the bank's bytes
               (the floor of a kernel that reads the bank once) and torch's own normalize -> matmul -> topk on the same
               tensors; and whether scores and rows came back bit-equal to the host's float32 fmaf chain.
One JSON line per measurement; --out writes them all to a file.
Usage on the GPU box: python tools/window_rate.py [--songs 16] [--iters 150] [--runs 5] [--one-clip] [--kernels] [--eval
                      [--eval-stride S]] [--transfer] [--styles] [--rotate] [--search] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'music-style-transfer_amd')]
import numpy as np
import torch

from tools.synth import synth_clip

C, T, BARS = 4, 4, 16


def synth_songs(n, seed=0):
    """`n` songs in get_input's form (float64 rolls), 24 to 64 bars long."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        R = int(rng.integers(24, 65))
        c = synth_clip(500 + k, C, R, T, True, density=.02, bpm=70 + 5 * (k % 20))
        info = dict(bpm=c['bpm_int'], scale=dict(mode='major' if k % 2 else 'minor'))
        out.append((f'synth{k}', (info, c['pitched'][0].double().numpy(), c['instruments_features'][0].double().numpy(),
                                  list(range(C)), c['unpitched'][0].double().numpy())))
    return out


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), runs=len(values))


def windowed(model, opt, store, K, iters, runs, warmup=4):
    rng = np.random.default_rng(0)

    def loop(n):
        for _ in range(n):
            model.train_windows(store, store.sample(rng, K, BARS))
            opt.step()
    loop(warmup)                                          # eager, capture + replay, replays
    torch.cuda.synchronize()
    rates = []
    for _ in range(runs):
        t0 = time.perf_counter()
        loop(iters)
        torch.cuda.synchronize()
        rates.append(K * iters / (time.perf_counter() - t0))
    model.check_device_status()
    return dict(what='train_windows + FusedAdam.step', K=K, bars=BARS, C=C, T=T, unit='clip-iterations/s', **spread(rates))


def one_clip(model, songs, iters, runs):
    from style.train import train
    cut = [(name, (info, p[:, :BARS], f, ins, u[:, :BARS])) for name, (info, p, f, ins, u) in songs]

    def feed(n):
        for i in range(n + 4):                            # (the prefetch thread runs a song or two ahead)
            yield cut[i % len(cut)]
    run = lambda n: train(model, feed(n), n_iterations=n, iter_size=2, training_info_path=None, save_path=None, progress=False,
                          fused=True, sparse_input=True)
    run(8)                                                # both lanes: eager, capture, replay
    torch.cuda.synchronize()
    rates = []
    for _ in range(runs):
        t0 = time.perf_counter()
        run(iters)
        torch.cuda.synchronize()
        rates.append(iters / (time.perf_counter() - t0))
    return dict(what='train(fused=True, sparse_input=True), songs cut to 16 bars', K=1, bars=BARS, C=C, T=T,
                unit='clip-iterations/s', **spread(rates))


def kernels(store, K, reps=50):
    """Microseconds of the crop of K clips (two mst_clip_window launches) and of mst_clip_scatter writing the same
    destinations from per-clip record buffers holding the same windows."""
    from style import _native
    from style.data import sparsify
    native, dev = _native.get(), store.device
    batch = store.sample(np.random.default_rng(1), K, BARS)
    win = torch.zeros(2, K, 4, dtype=torch.int32)
    store.describe(batch, win.numpy())
    win = win.to(dev)
    shapes = {5: (C, BARS, T * 560), 2: (1, BARS, T * 470)}
    outs = {n: torch.full((K,) + s + (n,), float('nan'), device=dev) for n, s in shapes.items()}
    stream = _native.current_stream(dev)

    def crop():
        for row, n in ((0, 5), (1, 2)):
            ch, bars, bar_cells = shapes[n]
            native.clip_window(store.pools[n].cells, store.pools[n].feats, win[row], outs[n], K, ch, bars, bar_cells, n, stream)
    crop()
    torch.cuda.synchronize()
    want = {n: o.clone() for n, o in outs.items()}
    # the same windows as per-clip record buffers, the layout mst_clip_scatter reads
    packs = {}
    for n in (5, 2):
        rolls = [sparsify(want[n][k].cpu(), pin=False) for k in range(K)]
        cap = max(r.count for r in rolls)
        cells, feats = torch.zeros(K, cap, dtype=torch.int32), torch.zeros(K, cap, n)
        for k, r in enumerate(rolls):
            cells[k, :r.count], feats[k, :r.count] = r.cells, r.feats
        packs[n] = (cells.to(dev), feats.to(dev), torch.tensor([r.count for r in rolls], dtype=torch.int32).to(dev), cap)

    def scatter():
        for n in (5, 2):
            cells, feats, counts, cap = packs[n]
            native.clip_scatter(cells, feats, counts, outs[n], int(np.prod(shapes[n])), n, n_clips=K, capacity=cap, stream=stream)
    for o in outs.values():
        o.fill_(float('nan'))
    scatter()
    torch.cuda.synchronize()
    assert all(torch.equal(outs[n].view(torch.int32), want[n].view(torch.int32)) for n in outs), 'crop and scatter disagree'
    nbytes = sum(o.numel() * 4 for o in outs.values())
    res = []
    for name, fn in (('mst_clip_window x 2', crop), ('mst_clip_scatter x 2', scatter), ('mst_clip_window x 2', crop),
                     ('mst_clip_scatter x 2', scatter)):                # alternated
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        res.append(dict(what=name, K=K, bytes_written=nbytes, unit='us', tb_per_s=nbytes / (statistics.median(times) * 1e-6) / 1e12,
                        **spread(times)))
    return res


def eval_rounds(model, store, K, stride, runs, rounds=3):
    """Windows per second of evaluate_windows rounds (host clock around `rounds` rounds; each ends in its one download)."""
    from style.train import evaluate_windows
    for _ in range(2):                                    # eager, then capture + replay (per plan)
        res = evaluate_windows(model, store, BARS, K, stride)
    torch.cuda.synchronize()
    n_batches = len(store.window_batches(BARS, K, stride))
    rates, ms = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(rounds):
            res = evaluate_windows(model, store, BARS, K, stride)
        dt = time.perf_counter() - t0
        rates.append(rounds * res['clips'] / dt)
        ms.append(dt / rounds * 1e3)
    model.check_device_status()
    return dict(what='evaluate_windows', K=K, bars=BARS, C=C, T=T, stride=stride or BARS, windows=res['clips'], batches=n_batches,
                windows_skipped=res['windows_skipped'], round_ms=spread(ms), unit='windows/s', **spread(rates))


def eval_per_song(model, songs, runs):
    """Songs per second of style.train.evaluate, one whole song per eval_iteration call, on the same songs."""
    from style.train import evaluate
    run = lambda: evaluate(model, iter(songs), len(songs), sparse_input=True)
    run()                                                 # builds the plan of every shape
    torch.cuda.synchronize()
    rates = []
    for _ in range(runs):
        t0 = time.perf_counter()
        res = run()
        rates.append(res['clips'] / (time.perf_counter() - t0))
    bars = sum(p.shape[1] for _, (_, p, _, _, _) in songs)
    return dict(what='evaluate(sparse_input=True), one song per call', songs=len(songs), bars=bars, C=C, T=T, unit='songs/s',
                **spread(rates))


def eval_kernels(model, store, K, reps=50):
    """Microseconds, under device events, of mst_window_inputs placing K clips' small inputs and of mst_eval_accumulate folding K
    clips."""
    from style import _native
    native, dev = _native.get(), store.device
    plan = model._plan(C, BARS, T, True, dev, clips=K)
    bucket = store.buckets[(C, T, True)]
    table = bucket['table']
    names = ('mode', 'bpm', 'instr', 'used_instruments', 'bpm_target')
    fields = _native.RowFields.of([(a, b - a, plan.slot(n)[0]) for n, (a, b) in zip(names, bucket['fields'])])
    ws = plan.new_ws()
    rows = torch.tensor([k % len(bucket['songs']) for k in range(K)], dtype=torch.int32, device=dev)
    losses = torch.rand(K, _native.N_LOSSES, device=dev)
    metrics = torch.rand(K, C + 2, _native.METRIC_WORDS, dtype=torch.float64, device=dev)
    live = torch.tensor([K], dtype=torch.int32, device=dev)
    acc = torch.zeros(_native.EVAL_ACC_WORDS, dtype=torch.float64, device=dev)
    stream = _native.current_stream(dev)
    calls = (('mst_window_inputs', lambda: native.window_inputs(table, table.shape[0], table.shape[1], rows, K, fields,
                                                                 plan.clip_stride, ws, stream)),
             ('mst_eval_accumulate', lambda: native.eval_accumulate(losses, metrics, K, C, live, acc, stream)))
    res = []
    for name, fn in calls + calls:                         # alternated
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        res.append(dict(what=name, K=K, C=C, unit='us', **spread(times)))
    return res


def thin_predictions(model, windows, density=.02):
    """A randomly initialised model predicts every velocity near .5: every cell a note, which no trained model does.  Scale the
    two appliers' last Linear by 20 and move their velocity bias so that `density` of the cells of `windows`, each rendered in
    another's style, pass hard_output's .01 threshold — the density of the songs themselves — so that the record buffers and the
    download are about those of real use.  (The density of a single clip still varies with its donor: TRANSFER_CAPACITY.)"""
    lift = np.log(.01 / .99)
    with torch.no_grad():
        for applier in (model.pitched_style_applier, model.unpitched_style_applier):
            applier.linear.weight *= 20.
        styles = [model.extract_style(*w)[0] for w in windows]
        logits = ([], [])
        for i, w in enumerate(windows):
            d = (i * 5 + 3) % len(windows)
            _, melody, rhythm = model.extract_style(*w)
            for x, into in zip(model.apply_style(styles[d], melody, rhythm, windows[d][3], True), logits):
                v = x[..., 1].double().clamp(1e-30, 1 - 1e-16).reshape(-1)
                into.append(torch.log(v / (1 - v)).float())
        for applier, rows in zip((model.pitched_style_applier, model.unpitched_style_applier), logits):
            applier.linear.bias[1] += float(lift - torch.quantile(torch.cat(rows), 1 - density))
    model._sync_flat()


TRANSFER_CAPACITY = C * BARS * T * 560 // 4     # records per clip and roll the --transfer legs leave room for


def transfer_legs(model, store, songs, clips, iters, runs):
    """Windows per second of StyleTransferModel.transfer_windows (every K of `clips`, with and without score; random windows and
    random donors; each call ends in its one synchronising read and the download of the records) against the per-window Python
    surface on device-resident dense windows of the same songs — extract_style, predict_song_info with a donor's style,
    apply_style with the donor's instruments, hard_output_sparse x 2: the only way to do this work before transfer_windows.
    All legs are warmed up, then timed in turn `runs` times (host clock around a window that ends synchronised)."""
    from style.data import prepare_input
    from style.model import hard_output_sparse
    rng = np.random.default_rng(0)
    windows = []
    for name, (info, p, f, ins, u) in songs[:8]:
        r0 = int(rng.integers(0, p.shape[1] - BARS + 1))
        windows.append(prepare_input((name, (info, p[:, r0:r0 + BARS], f, ins, u[:, r0:r0 + BARS]))))
    thin_predictions(model, windows)

    def batched(K, score):
        def run(n):
            for _ in range(n):
                res = model.transfer_windows(store, store.sample(rng, K, BARS), rng.integers(0, K, K), score=score, capacity=TRANSFER_CAPACITY)
            return K * n, res
        return run

    styles = []

    def surface(n):
        with torch.no_grad():
            if not styles:
                styles.extend(model.extract_style(*w)[0] for w in windows)
            for i in range(n):
                w, d = windows[i % len(windows)], (i * 5 + 3) % len(windows)
                _, melody, rhythm = model.extract_style(*w)
                model.predict_song_info(styles[d], rhythm)
                xp, xu = model.apply_style(styles[d], melody, rhythm, windows[d][3], True)
                res = hard_output_sparse(xp), hard_output_sparse(xu)
        return n, res
    legs = [(f'transfer_windows, K = {K}' + (', score' if score else ''), batched(K, score), max(iters // K, 4)) for K in clips
            for score in (False, True)]
    legs.append(('extract_style / predict_song_info / apply_style / hard_output_sparse per window', surface, iters))
    rates = {name: [] for name, _, _ in legs}
    records = {}
    for name, run, n in legs:                              # eager, capture + replay, replays; the plans of every shape
        _, res = run(3)
        torch.cuda.synchronize()
        rolls = res.pitched + res.unpitched if hasattr(res, 'pitched') else list(res)
        records[name] = sum(r.count for r in rolls) / (len(rolls) / 2)
    for _ in range(runs):
        for name, run, n in legs:                          # interleaved
            t0 = time.perf_counter()
            done, _ = run(n)
            torch.cuda.synchronize()
            rates[name].append(done / (time.perf_counter() - t0))
    model.check_device_status()
    return [dict(what=name, bars=BARS, C=C, T=T, records_per_window=records[name], unit='windows/s', **spread(rates[name]))
            for name, _, _ in legs]


def transfer_kernels(model, store, K, reps=50):
    """Microseconds, under device events, of the calls transfer_windows adds to the existing ones, at K clips: mst_clip_gather of
    the style vectors (one launch), mst_rolls_count (two launches) and mst_rolls_compact (one) on the K pitched predictions of
    a batched plan's workspace, and mst_style_sums (one launch)."""
    from style import _native
    native, dev = _native.get(), model._anchor().device     # (the device the model keys its plans by)
    plan = model._plan(C, BARS, T, True, dev, clips=K)
    model.transfer_windows(store, store.sample(np.random.default_rng(2), K, BARS), list(range(K)),
                           capacity=TRANSFER_CAPACITY)                                                  # fills a workspace
    st = plan.__dict__['_transfer_window_state']
    ws, bank = st['ws'], st['bank']
    style_off, _, size = plan.slot('style')
    slots = ws.data_ptr() + 4 * style_off
    idx = torch.tensor([(k * 5 + 3) % K for k in range(K)], dtype=torch.int32, device=dev)
    n_cells = C * BARS * T * 560
    x = ws.data_ptr() + 4 * plan.slot('pitched_pred')[0]
    rws = torch.empty(K, native.roll_slices(n_cells) + 1, dtype=torch.int32, device=dev)
    cap = TRANSFER_CAPACITY
    cells, feats = torch.empty(K, cap, dtype=torch.int32, device=dev), torch.empty(K, cap, 5, device=dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    sums = torch.empty(K, _native.STYLE_SUM_WORDS, dtype=torch.float64, device=dev)
    stream = _native.current_stream(dev)
    calls = (('mst_clip_gather', lambda: native.clip_gather(bank, K, size, slots, plan.clip_stride, idx, K, size, stream)),
             ('mst_rolls_count (2 launches)', lambda: native.rolls_count(x, plan.clip_stride, K, n_cells, 5, 1, rws, stream)),
             ('mst_rolls_compact', lambda: native.rolls_compact(x, plan.clip_stride, K, n_cells, 5, 1, rws, cap, cells, feats, counts, stream)),
             ('mst_style_sums', lambda: native.style_sums(slots, plan.clip_stride, bank, K, size, idx, K, size, sums, stream)))
    res = []
    for name, fn in calls + calls:                         # alternated
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        res.append(dict(what=name, K=K, C=C, style_size=size, roll_cells=n_cells, unit='us', **spread(times)))
    return res


def style_legs(model, store, songs, clips, iters, runs):
    """Windows per second of encode_styles (a whole pass over the store per call), of transfer_styles (each clip a blend of two
    songs' mean styles out of the bank, instruments decided per clip on the device) and of transfer_windows at the same K on the
    same random windows, and of the per-window Python surface doing transfer_styles' work with the decision on the host:
    extract_style, predict_song_info, select_instruments + encode_instruments (a download in the middle), apply_style,
    hard_output_sparse x 2.  All legs are warmed up, then timed in turn `runs` times."""
    from style.data import encode_instruments, prepare_input
    from style.model import hard_output_sparse
    from style.style_transfer import select_instruments
    rng = np.random.default_rng(0)
    windows = []
    for name, (info, p, f, ins, u) in songs[:8]:
        r0 = int(rng.integers(0, p.shape[1] - BARS + 1))
        windows.append(prepare_input((name, (info, p[:, r0:r0 + BARS], f, ins, u[:, r0:r0 + BARS]))))
    thin_predictions(model, windows)
    dev = model._anchor().device
    banks = {}

    def encode(K):
        def run(n):
            for _ in range(n):
                banks[K] = model.encode_styles(store, BARS, K)
            return n * len(banks[K]), None
        return run

    def styles(K):
        def run(n):
            bank, ids = banks[K], sorted(banks[K].by_song)
            for _ in range(n):
                mix = [bank.blend([(ids[int(a)], .5), (ids[int(b)], .5)]) for a, b in rng.integers(0, len(ids), (K, 2))]
                res = model.transfer_styles(store, store.sample(rng, K, BARS), bank, mix, instruments='each', capacity=TRANSFER_CAPACITY)
            return K * n, res
        return run

    def plain(K):
        def run(n):
            for _ in range(n):
                res = model.transfer_windows(store, store.sample(rng, K, BARS), rng.integers(0, K, K), capacity=TRANSFER_CAPACITY)
            return K * n, res
        return run
    kept = []

    def surface(n):
        with torch.no_grad():
            if not kept:
                kept.extend(model.extract_style(*w)[0] for w in windows)
            for i in range(n):
                w, d = windows[i % len(windows)], (i * 5 + 3) % len(windows)
                style = kept[d] * .5 + kept[(d + 1) % len(windows)] * .5
                _, melody, rhythm = model.extract_style(*w)
                ip, _, _ = model.predict_song_info(style, rhythm)
                programs, _ = select_instruments(ip.cpu().numpy()[0], C + 1)
                feats = torch.tensor(encode_instruments(programs[:C]), dtype=torch.float).to(dev).unsqueeze(0)
                xp, xu = model.apply_style(style, melody, rhythm, feats, True)
                res = hard_output_sparse(xp), hard_output_sparse(xu)
        return n, res
    legs = []
    for K in clips:
        legs += [(f'encode_styles, K = {K}', encode(K), 2), (f'transfer_styles, K = {K}', styles(K), max(iters // K, 4)),
                 (f'transfer_windows, K = {K}', plain(K), max(iters // K, 4))]
    legs.append(('extract_style / predict_song_info / select_instruments / apply_style / hard_output_sparse per window', surface, iters))
    rates = {name: [] for name, _, _ in legs}
    for name, run, n in legs:                              # eager, capture + replay, replays; the plans of every shape
        run(3)
        torch.cuda.synchronize()
    for _ in range(runs):
        for name, run, n in legs:                          # interleaved
            t0 = time.perf_counter()
            done, _ = run(n)
            torch.cuda.synchronize()
            rates[name].append(done / (time.perf_counter() - t0))
    model.check_device_status()
    return [dict(what=name, bars=BARS, C=C, T=T, unit='windows/s', **spread(rates[name])) for name, _, _ in legs]


def style_kernels(model, store, K, entries=8, reps=50):
    """Microseconds, under device events, of the three launches the style bank adds, at K clips: mst_style_put of the K style
    slots into a bank, mst_style_mix of `entries` rows per clip back into them, and mst_info_decide on the K predictions."""
    from style import _native
    from style.data import group_of_instrument
    native, dev = _native.get(), model._anchor().device
    plan = model._plan(C, BARS, T, True, dev, clips=K)
    ws = plan.new_ws()
    ws[:K * plan.clip_stride].uniform_(-1, 1)
    slot = lambda name: ws.data_ptr() + 4 * plan.slot(name)[0]
    size = plan.slot('style')[2]
    bank = torch.zeros(4 * K, size, device=dev)
    rows = torch.arange(K, dtype=torch.int32, device=dev)
    offsets = torch.arange(0, (K + 1) * entries, entries, dtype=torch.int32, device=dev)
    idx = torch.randint(0, K, (K * entries,), dtype=torch.int32, device=dev)
    w = torch.full((K * entries,), 1. / entries, device=dev)
    rec = torch.zeros(K, C + 2, dtype=torch.int32, device=dev)
    stream = _native.current_stream(dev)
    n_logits = plan.slot('instruments_pred')[2]
    calls = (('mst_style_put', lambda: native.style_put(slot('style'), plan.clip_stride, bank, 4 * K, size, rows, K, size, stream)),
             (f'mst_style_mix, {entries} entries per clip', lambda: native.style_mix(bank, 4 * K, size, offsets, idx, w, K * entries, slot('style'),
                                                                                     plan.clip_stride, K, size, stream)),
             ('mst_info_decide', lambda: native.info_decide(slot('instruments_pred'), slot('mode_pred'), slot('bpm_pred'), plan.clip_stride,
                                                            n_logits, group_of_instrument, plan.slot('instr')[2] // C - (n_logits - 1), C, K,
                                                            False, None, slot('instr'), slot('mode'), slot('bpm'), plan.clip_stride, rec,
                                                            stream)))
    res = []
    for name, fn in calls + calls:                         # alternated
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        res.append(dict(what=name, K=K, C=C, style_size=size, unit='us', **spread(times)))
    return res


def rotate_legs(model, opt, ring, fresh, K, E, M, iters, runs, warmup=4):
    """Clip-iterations per second of the loop with and without refresh, alternated; `fresh` is an endless source of
    pre-sparsified songs."""
    rngs = {True: np.random.default_rng(0), False: np.random.default_rng(0)}
    spent = []

    def loop(n, refresh):
        rng = rngs[refresh]
        for i in range(n):
            model.train_windows(ring, ring.sample(rng, K, BARS))
            opt.step()
            if refresh and (i + 1) % E == 0:
                t0 = time.perf_counter()
                ring.admit([next(fresh) for _ in range(M)])
                spent.append(time.perf_counter() - t0)
    for refresh in (False, True):
        loop(max(warmup, E), refresh)                     # eager, capture + replay, replays; the staging buffers of admit
    torch.cuda.synchronize()
    spent.clear()
    rates = {False: [], True: []}
    for _ in range(runs):
        for refresh in (False, True):                     # alternated
            t0 = time.perf_counter()
            loop(iters, refresh)
            torch.cuda.synchronize()
            rates[refresh].append(K * iters / (time.perf_counter() - t0))
    ring.check()
    model.check_device_status()
    ratio = statistics.median(rates[True]) / statistics.median(rates[False])
    return [dict(what='train_windows + FusedAdam.step, no refresh', K=K, bars=BARS, unit='clip-iterations/s', **spread(rates[False])),
            dict(what=f'the same with SongStore.admit of {M} songs after every {E}th iteration', K=K, E=E, M=M, bars=BARS,
                 unit='clip-iterations/s', ratio_to_no_refresh=ratio, admit_host_us=spread([t * 1e6 for t in spent]), **spread(rates[True]))]


def rotate_kernels(ring, clips, reps=50):
    """Microseconds under device events of one refresh of `clips`: the mst_store_admit launch alone (the blob already staged),
    the whole `admit` (pack, upload, launch), the separate copies of `add` into an append-only store, and one device-to-device
    copy of the same bytes."""
    from style import _native
    from style.data import SongStore
    native, dev = _native.get(), ring.device
    ring.admit(clips)
    torch.cuda.synchronize()
    ring.check()
    key = ring.songs[ring.resident()[-1]]['key']
    dsts = _native.AdmitDsts([ring.pools[5].cells, ring.pools[5].feats, ring.pools[2].cells, ring.pools[2].feats, ring.buckets[key]['table']])
    words = sum(c.pitched_channels.count * 6 + c.unpitched_channels.count * 3 for c in clips) + len(clips) * ring.buckets[key]['table'].shape[1]
    stream = _native.current_stream(dev)
    src, dst = torch.zeros(words, dtype=torch.int32, device=dev), torch.zeros(words, dtype=torch.int32, device=dev)
    plain = SongStore(dev, capacity=1 << 22)

    def adds():
        for c in clips:
            plain.add(c)
    calls = (('mst_store_admit launch', lambda: native.store_admit(ring._blob, ring._blob.numel(), ring._max_segments, dsts, ring._status[0], stream)),
             ('SongStore.admit (pack, upload, launch)', lambda: ring.admit(clips)),
             (f'SongStore.add x {len(clips)} (append-only: {5 * len(clips)} copies)', adds),
             ('device-to-device copy of the same bytes', lambda: dst.copy_(src)))
    res = []
    for name, fn in calls + calls:                         # alternated
        fn()
        torch.cuda.synchronize()
        times, host = [], []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            host.append((time.perf_counter() - t0) * 1e6)
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        res.append(dict(what=name, songs=len(clips), bytes=4 * words, unit='us', host_us=spread(host),
                        gb_per_s=4 * words / (statistics.median(times) * 1e-6) / 1e9, **spread(times)))
    ring.check()
    return res


def rotate(model, opt, songs, clips, iters, runs):
    from style.train import Rotation, iter_sparse
    resident = [c for c in iter_sparse(iter(songs)) if c is not None]
    more = [c for c in iter_sparse(iter(synth_songs(16, seed=1))) if c is not None]

    def endless():
        while True:
            yield from more
    results = []
    for K in clips:
        for E, M in ((16, 4), (4, 4)):
            ring = Rotation(iter(resident), E, M).first_store(len(resident))
            results += rotate_legs(model, opt, ring, endless(), K, E, M, iters, runs)
    results += rotate_kernels(ring, more[:4])
    return results


def host_chain(queries, bank):
    """mst_amd.h's score of every (query, row) pair on the host: the float32 fmaf chains (the product of two floats is exact in
    float64, so float32(float64 product + float64 acc) is the fma), np.sqrt and / in float32."""
    def dots(a, b):
        acc = np.zeros((len(a), len(b)), dtype=np.float32)
        for i in range(a.shape[1]):
            acc = (a[:, i, None].astype(np.float64) * b[None, :, i].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        return acc

    def squares(a):
        acc = np.zeros(len(a), dtype=np.float32)
        for i in range(a.shape[1]):
            acc = (a[:, i].astype(np.float64) ** 2 + acc.astype(np.float64)).astype(np.float32)
        return acc
    return dots(queries, bank) / (np.sqrt(squares(queries))[:, None] * np.sqrt(squares(bank))[None, :])


def search_kernels(N, D=256, Q=64, k=8, reps=50):
    """Microseconds, under device events, of mst_style_search (Q queries, N rows of D floats, the k nearest), of a copy of the
    bank's bytes and of torch's normalize -> matmul -> topk, alternated; the call's two launches apart from torch.profiler; and
    the comparison of scores and rows with the host chain."""
    from style import _native
    native, dev = _native.get(), torch.device('cuda:0')
    g = torch.Generator().manual_seed(N)
    bank = torch.randn(N, D, generator=g).to(dev)
    queries = torch.randn(Q, D, generator=g).to(dev)
    other = torch.empty_like(bank)
    rows = torch.empty(Q, k, dtype=torch.int32, device=dev)
    scores = torch.empty(Q, k, device=dev)
    scratch = torch.empty(native.style_search_scratch_bytes(N, Q, k) // 8, dtype=torch.int64, device=dev)
    stream = _native.current_stream(dev)
    search = lambda: native.style_search(bank, N, D, None, None, queries, Q, D, None, D, k, 1, rows, scores, scratch, stream)

    def by_torch():
        cos = torch.nn.functional.normalize(queries, dim=1) @ torch.nn.functional.normalize(bank, dim=1).T
        return torch.topk(cos, k, dim=1)
    calls = (('mst_style_search', search), ('device-to-device copy of the bank', lambda: other.copy_(bank)),
             ('torch normalize -> matmul -> topk', by_torch))
    res = []
    for name, fn in calls + calls:                         # alternated
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        res.append(dict(what=name, N=N, D=D, Q=Q, k=k, bank_bytes=4 * N * D, unit='us', **spread(times)))
    launches = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                search()
            torch.cuda.synchronize()
        for e in prof.events():
            if 'style_search' in e.name:
                launches.setdefault('merge' if 'merge' in e.name else 'scores and slab selection', []).append(float(e.device_time))
    except Exception as err:                               # the split is a report, not a dependency
        launches = {'error': [repr(err)]}
    res.append(dict(what='mst_style_search by launch (torch.profiler kernel durations)', N=N, D=D, Q=Q, k=k, unit='us',
                    **{name: spread(t) if t and not isinstance(t[0], str) else t for name, t in launches.items()}))
    search()
    torch.cuda.synchronize()
    got_rows, got_scores = rows.cpu().numpy(), scores.cpu().numpy()
    want = host_chain(queries.cpu().numpy(), bank.cpu().numpy())
    order = np.lexsort((np.broadcast_to(np.arange(N), want.shape), -want), axis=1)[:, :k]          # descending, ties by row
    torch_rows = by_torch()[1].cpu().numpy()
    res.append(dict(what='mst_style_search against the host chain', N=N, D=D, Q=Q, k=k,
                    scores_bit_equal=bool(np.array_equal(got_scores.view(np.uint32), np.take_along_axis(want, got_rows.astype(np.int64), 1).view(np.uint32))),
                    rows_equal=bool(np.array_equal(got_rows, order)), rows_equal_to_torch_topk=bool(np.array_equal(got_rows, torch_rows))))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--songs', type=int, default=16)
    ap.add_argument('--iters', type=int, default=150)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--clips', type=int, nargs='*', default=[8, 64])
    ap.add_argument('--one-clip', action='store_true')
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--eval', action='store_true')
    ap.add_argument('--eval-stride', type=int, default=None)
    ap.add_argument('--transfer', action='store_true')
    ap.add_argument('--styles', action='store_true')
    ap.add_argument('--rotate', action='store_true')
    ap.add_argument('--search', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('window_rate.py measures on the GPU; there is none here')
    if args.search:
        results = [r for N in (4096, 65536) for r in search_kernels(N)]
        for r in results:
            print(json.dumps(r))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.writelines(json.dumps(r) + '\n' for r in results)
        return
    from style.optim import FusedAdam
    from style.train import build_model, fill_store
    songs = synth_songs(args.songs)
    store = fill_store(iter(songs), len(songs))
    results = []
    if args.kernels:
        results += kernels(store, 64)
    model = build_model(seed=108)
    if args.eval:
        for K in args.clips:
            results.append(eval_rounds(model, store, K, args.eval_stride, args.runs))
        results.append(eval_per_song(model, songs, args.runs))
        results += eval_kernels(model, store, 64)
    if args.transfer:
        results += transfer_legs(model, store, songs, args.clips, args.iters, args.runs)
        results += transfer_kernels(model, store, 64)
    if args.styles:
        results += style_legs(model, store, songs, args.clips, args.iters, args.runs)
        results += style_kernels(model, store, 64)
    opt = FusedAdam(model)
    opt.zero_grad()
    if args.rotate:
        results += rotate(model, opt, songs, args.clips, args.iters, args.runs)
    for K in [] if args.eval or args.transfer or args.styles or args.rotate else args.clips:
        results.append(windowed(model, opt, store, K, args.iters, args.runs))
    if args.one_clip:
        results.append(one_clip(build_model(seed=108), songs, args.iters * 16, args.runs))
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.writelines(json.dumps(r) + '\n' for r in results)


if __name__ == '__main__':
    main()
