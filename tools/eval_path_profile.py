#!/usr/bin/env python3
"""Developer tool: what a held-out evaluation iteration costs on the card.  On the bench clip (C, R, T) = (4, 16, 4) at FULL
widths, as a one-clip plan and as a 64-clip plan, HIP events around --reps back-to-back calls (after a warm-up) of
  mst_eval_iteration     forward + loss + note metrics
  mst_train_iteration    the same plan's training iteration, for scale
  mst_forward            the forward pass alone
  metrics launches       mst_roll_metrics on the plan's pitched prediction (C groups per clip) and its unpitched one
  mst_roll_count         the count + scan launches on the same pitched roll: the same access pattern with ONE operand, so about
                         twice its time is what the pitched metrics launches are expected to take
Needs a GPU: there is no fallback.  One JSON line per clip count; --out writes them to a file.
Usage on the GPU box: python tools/eval_path_profile.py [--reps 10] [--clips 1 64] [--out profiles/eval_path_x.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'music-style-transfer_amd')]
import numpy as np
import torch

from tools.synth import synth_clip

FULL = dict(beat=64, bar=128, nrf=8, style=256, melody=8, rhythm=32)


def timed(launch, reps, warmup=3):
    """Microseconds per call: HIP events around `reps` back-to-back calls."""
    for _ in range(warmup):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 1)


def profile(K, reps, C=4, R=16, T=4):
    from style import _native as nat
    native, dev = nat.get(), torch.device('cuda:0')
    dims = nat.Dims(C=C, R=R, T=T, instr=51, n_instruments=41, has_unpitched=1, clips=K, **FULL)
    plan = nat.Plan(native, dims, dev)
    g = torch.Generator().manual_seed(0)
    params = torch.zeros(native.param_floats(dims))
    for name, off, shape in native.param_table(dims):
        n = int(np.prod(shape))
        fan = shape[1] * (shape[2] if len(shape) > 2 else 1) if len(shape) > 1 else shape[0]
        params[off:off + n] = (torch.rand(n, generator=g) * 2 - 1) / fan ** .5
    params = params.to(dev)
    gparams = torch.zeros_like(params)
    clips = [synth_clip(10 + k, C, R, T, True) for k in range(K)]
    for k, clip in enumerate(clips):
        plan.set_inputs(mode=clip['mode'], bpm=clip['bpm'], instr=clip['instruments_features'], used=clip['used_instruments'],
                        bpm_target=float(clip['bpm_int']), clip=k)
    xp = torch.cat([c['pitched'] for c in clips]).contiguous().to(dev)
    xu = torch.cat([c['unpitched'] for c in clips]).contiguous().to(dev)
    losses = torch.zeros(K, nat.N_LOSSES, device=dev)
    metrics = torch.zeros(K, C + 2, nat.METRIC_WORDS, dtype=torch.float64, device=dev)
    stream = nat.current_stream(dev)
    out = dict(clips=K, crt=[C, R, T], reps=reps)
    out['eval_iteration_us'] = timed(lambda: plan.eval_iteration(params, xp, xu, losses, metrics), reps)
    out['train_iteration_us'] = timed(lambda: plan.train_iteration(params, gparams, xp, xu, losses), reps)
    out['forward_us'] = timed(lambda: plan.forward(nat.STAGE_ALL, params, xp, xu), reps)
    # the metrics launches on their own, on dense copies of the predictions
    cells_p, cells_u = R * T * 560, R * T * 470
    pp = torch.stack([plan.view('pitched_pred', clip=k) for k in range(K)]).contiguous()
    up = torch.stack([plan.view('unpitched_pred', clip=k) for k in range(K)]).contiguous()
    scratch = torch.empty(native.roll_metrics_scratch_bytes(K * C, cells_p) // 8, dtype=torch.float64, device=dev)
    rec = torch.empty(K * C, nat.METRIC_WORDS, dtype=torch.float64, device=dev)
    out['pitched_metrics_us'] = timed(lambda: native.roll_metrics(pp, xp, K * C, cells_p, 5, scratch, rec, stream), reps)
    out['unpitched_metrics_us'] = timed(lambda: native.roll_metrics(up, xu, K, cells_u, 2, scratch, rec, stream), reps)
    ws = torch.empty(native.roll_slices(K * C * cells_p) + 1, dtype=torch.int32, device=dev)
    out['pitched_roll_count_us'] = timed(lambda: native.roll_count(pp, K * C * cells_p, 5, nat.ROLL_HARD, ws, stream), reps)
    out['pitched_roll_bytes'] = K * C * cells_p * 20
    plan.check_status()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--clips', type=int, nargs='+', default=[1, 64])
    ap.add_argument('--out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('eval_path_profile needs a GPU')
    lines = [json.dumps(profile(K, args.reps)) for K in args.clips]
    print('\n'.join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
