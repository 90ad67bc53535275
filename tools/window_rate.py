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
One JSON line per measurement; --out writes them all to a file.
Usage on the GPU box: python tools/window_rate.py [--songs 16] [--iters 150] [--runs 5] [--one-clip] [--kernels] [--eval
                      [--eval-stride S]] [--out FILE]"""
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
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('window_rate.py measures on the GPU; there is none here')
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
    opt = FusedAdam(model)
    opt.zero_grad()
    for K in [] if args.eval else args.clips:
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
