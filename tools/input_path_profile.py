#!/usr/bin/env python3
"""Developer tool: what feeding the training loop costs.  Times the fused loop (StyleTransferModel.train_iteration +
FusedAdam.step every second call, as style.train.train runs it) in iterations per second when every iteration gets a clip
from the HOST, two ways:
  dense   style.data.prepare_input per iteration: float64 -> float32 on the loop thread, pageable H2D copy of the rolls,
          device-to-device copy into the lane's static buffers;
  sparse  style.data.prepare_input_sparse done ahead (the prefetch thread's work in train(sparse_input=True)); per iteration
          only the upload of the note records and mst_clip_scatter.
Shapes: the bench clip (synthetic, density 0.02) and two real songs of tests/golden/midi cut to the 800 // C bars train() cuts
them to.  The host clips are made before timing (parsing is outside the timed region) and rotate, so no iteration uploads the
clip it has just seen.  Also: the scatter launch under HIP events (bytes written per second against the 6.29 TB/s float4-copy
rate of the card), the record bytes against the dense bytes, and the host time of sparsify.
One JSON line per shape and feed; --out writes them all to a file.  --no-sparse runs the dense legs only (it then needs nothing
of the sparse path, so the same file measures an older tree).
Usage on the GPU box: python tools/input_path_profile.py [--runs 6] [--iters 40] [--no-sparse] [--out profiles/input_path_x.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'music-style-transfer_amd')]
import numpy as np
import torch

from bench import CLIP
from tools.synth import synth_clip

MIDI = os.path.join(ROOT, 'tests', 'golden', 'midi')
REAL = ['Kashmir.2.mid', 'Welcome to the Jungle.2 (300 it).mid']
COPY_ROOF = 6.29e12            # bytes / s, float4 copy on this card
ROTATION = 4                   # distinct host clips per shape


def bench_songs():
    """The bench clip's shape in get_input's form (float64 rolls), ROTATION different clips."""
    out = []
    for k in range(ROTATION):
        c = synth_clip(100 + k, CLIP['C'], CLIP['R'], CLIP['T'], True, density=.02)
        info = dict(bpm=c['bpm_int'], scale=dict(mode='major'))
        out.append((f'bench{k}', (info, c['pitched'][0].double().numpy(), c['instruments_features'][0].double().numpy(),
                                   list(range(CLIP['C'])), c['unpitched'][0].double().numpy())))
    return out


def real_songs(name):
    """One parsed song and ROTATION - 1 variants of the same shape (its bars rotated), so that the clips differ."""
    from style.style_transfer import get_model_input
    path, (info, pitched, feats, instruments, unpitched) = get_model_input(os.path.join(MIDI, name))
    out = []
    for k in range(ROTATION):
        shift = 7 * k
        out.append((path, (info, np.roll(pitched, shift, axis=1), feats, instruments,
                           None if unpitched is None else np.roll(unpitched, shift, axis=1))))
    return out


def timed_loop(model, opt, feed, iters, warmup):
    """Iterations per second of the fused loop; feed(i) returns train_iteration's arguments for iteration i."""
    for i in range(warmup):
        model.train_iteration(*feed(i))
        if i % 2:
            opt.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        model.train_iteration(*feed(warmup + i))
        if i % 2:
            opt.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    model.check_device_status()
    return iters / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=6)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--no-sparse', action='store_true')
    ap.add_argument('--shapes', default='bench,real', help='comma list of: bench, real')
    ap.add_argument('--tag', default='', help='copied into every JSON line (which tree this is)')
    ap.add_argument('--out')
    args = ap.parse_args()

    from style.data import prepare_input, get_used_instruments
    from style.optim import FusedAdam
    from style.train import build_model
    dev = torch.device('cuda:0')
    model = build_model(seed=108)
    opt = FusedAdam(model)
    shapes = []
    if 'bench' in args.shapes:
        shapes.append(('bench', bench_songs()))
    if 'real' in args.shapes:
        shapes += [(name, real_songs(name)) for name in REAL]
    lines = []
    for name, songs in shapes:
        C = songs[0][1][1].shape[0]
        cap = 800 // C

        def dense_feed(i):
            song = songs[i % len(songs)]
            mode, bpm, pitched, features, unpitched = prepare_input(song, cap)
            return mode, bpm, pitched, features, unpitched, get_used_instruments(features, unpitched), song[1][0]['bpm']

        feeds = [('dense', dense_feed)]
        extra = {}
        if not args.no_sparse:
            from style.data import prepare_input_sparse
            from style.train import SmallInputStager
            stager = SmallInputStager(dev)
            from style.sparse import scatter_packed
            from style import _native
            t0 = time.perf_counter()
            clips = [prepare_input_sparse(song, cap) for song in songs]
            extra['host_sparsify_ms_per_clip'] = round((time.perf_counter() - t0) * 1e3 / len(songs), 2)

            def sparse_feed(i):
                clip = clips[i % len(clips)]
                mode, bpm, pitched, features, unpitched = clip
                mode, bpm, features, used = stager.upload(mode, bpm, features, get_used_instruments(features, unpitched))
                return mode, bpm, pitched, features, unpitched, used, clip.bpm_target

            feeds.append(('sparse', sparse_feed))
            # the scatter launch on its own: records resident, HIP events around `reps` launches
            kernel = []
            for roll in (clips[0].pitched_channels, clips[0].unpitched_channels):
                if roll is None:
                    continue
                records = roll.packed.to(dev)
                out = torch.full(roll.shape, float('nan'), device=dev)
                stream = _native.current_stream(dev)
                launch = lambda: scatter_packed(_native.get(), records, roll.count, roll.n_cells, roll.nfeat, out, stream)
                for _ in range(5):
                    launch()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                reps = 50
                e0.record()
                for _ in range(reps):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / reps
                dense_bytes = roll.n_cells * roll.nfeat * 4
                kernel.append(dict(nfeat=roll.nfeat, records=roll.count, us=round(us, 2), dense_bytes=dense_bytes,
                                   record_bytes=roll.packed.numel() * 4, written_tb_s=round(dense_bytes / us / 1e6, 3),
                                   of_copy_roof=round(dense_bytes / (us * 1e-6) / COPY_ROOF, 3)))
                del out, records
            extra['scatter'] = kernel
        for feed_name, feed in feeds:
            runs = [round(timed_loop(model, opt, feed, args.iters, args.warmup), 1) for _ in range(args.runs)]
            shape = tuple(int(d) for d in songs[0][1][1][:, :cap].shape[:3])
            line = dict(tag=args.tag, shape_name=name, crt=shape, feed=feed_name, iters=args.iters, it_per_s=runs,
                        median=float(np.median(runs)), min=min(runs), max=max(runs), **(extra if feed_name == 'sparse' else {}))
            print(json.dumps(line), flush=True)
            lines.append(line)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(lines, f, indent=1)


if __name__ == '__main__':
    main()
