#!/usr/bin/env python3
"""Developer tool: what the guarded optimizer step (FusedAdam(max_grad_norm=..., skip_nonfinite=...), mst_adam_step_guarded)
costs on the card.  Two measurements:
  kernels  HIP-event time of mst_adam_step2 against mst_adam_step_guarded at the full-width model's flat size (n = 980 325,
           with grads2): 200 back-to-back calls each, the two alternating, --runs rounds; microseconds per call.
  loop     the rate of the fused loop (StyleTransferModel.train_iteration twice, then FusedAdam.step) on the bench clip,
           seed-108 weights, with the guard off and on, alternating in one process; iterations per second.
Yardstick of the loop: the parent commit's build in the same job.  --parent DIR names a built checkout of the parent; a
child process per tree and run takes the loop measurement with that tree's package (the parent's knows no guard: off only),
parent and this tree alternating, --runs times each; the spread of the parent's own runs stands beside every difference.
Needs a GPU: there is no fallback.  Prints one JSON document; --out writes it to a file as well.
Usage on the GPU box: python tools/guarded_step_profile.py [--parent DIR] [--runs 6] [--out profiles/guarded_step.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FULL = 980325
HYPER = (.01, .9, .999, 1e-8, 200, .9)
CLIP = dict(C=4, R=16, T=4)             # bench.py's clip


def spread(values, digits=2):
    import numpy as np
    return dict(median=round(float(np.median(values)), digits), min=round(min(values), digits), max=round(max(values), digits))


def kernels_leg(runs, calls=200):
    import torch
    from style import _native
    lib, dev = _native.get().lib, torch.device('cuda:0')
    n = N_FULL
    mk = lambda: torch.zeros(n, device=dev)
    p, m, v, state, guard = torch.randn(n, device=dev), mk(), mk(), torch.zeros(4, device=dev), torch.zeros(8, device=dev)
    g, g2 = torch.randn(n, device=dev) * 1e-3, torch.randn(n, device=dev) * 1e-3
    scratch = torch.zeros(lib.mst_grad_guard_scratch_bytes(n) // 8, dtype=torch.float64, device=dev)
    P, s = (lambda t: t.data_ptr()), _native.current_stream(dev)
    # zero_grad = 0: every call sees the same gradient (clipped to half its norm by the guarded leg)
    plain = lambda: lib.mst_adam_step2(P(p), P(g), P(g2), P(m), P(v), n, P(state), *HYPER, 0, s)
    max_norm = float((g + g2).norm()) / 2
    guarded = lambda: lib.mst_adam_step_guarded(P(p), P(g), P(g2), P(m), P(v), n, P(state), P(guard), P(scratch), *HYPER,
                                                max_norm, 1, 0, s)
    us = dict(adam_step2=[], adam_step_guarded=[])
    for fn in (plain, guarded):
        for _ in range(10):
            assert fn() == 0
    for _ in range(runs):                                  # the two alternate
        for name, fn in (('adam_step2', plain), ('adam_step_guarded', guarded)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    w = guard.cpu().tolist()
    return dict(n=n, calls=calls, runs=runs, us_per_call={k: spread(x) for k, x in us.items()},
                steps_clipped=int(w[4]), steps_skipped=int(w[3]))


def loop_leg(iters, warm, guards):
    """iterations / s of the fused loop for every entry of `guards` ('off' / 'on'), in the order given."""
    import torch
    from style.optim import FusedAdam
    from style.train import build_model
    from tools.synth import synth_clip
    dev = torch.device('cuda:0')
    c = {k: (t.to(dev) if torch.is_tensor(t) else t) for k, t in synth_clip(0, CLIP['C'], CLIP['R'], CLIP['T'], True).items()}
    out = []
    for guard in guards:
        model = build_model().to(dev)                     # seed-108 weights for every leg
        opt = FusedAdam(model, lr=.01, step_size=200, gamma=.9, **(dict(max_grad_norm=1., skip_nonfinite=True) if guard == 'on' else {}))

        def body(it):
            model.train_iteration(c['mode'], c['bpm'], c['pitched'], c['instruments_features'], c['unpitched'], c['used_instruments'],
                                  c['bpm_int'])
            if (it + 1) % 2 == 0:
                opt.step()
        for it in range(warm):
            body(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(iters):
            body(it)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        line = dict(guard=guard, iters=iters, iters_per_s=round(iters / dt, 1), us_per_pair=round(2e6 * dt / iters, 1))
        if guard == 'on':
            line['guard_stats'] = opt.guard_stats()
        out.append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=6)
    ap.add_argument('--iters', type=int, default=2000, help='loop iterations per timed window')
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--parent', help='a built checkout of the parent commit: the yardstick of the loop measurement')
    ap.add_argument('--out')
    ap.add_argument('--child', nargs='+', metavar='GUARD', help=argparse.SUPPRESS)      # one loop measurement of --tree
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:                                         # the only processes that open the GPU
        sys.path[:0] = [args.tree, os.path.join(args.tree, 'music-style-transfer_amd')]
        import torch
        if not torch.cuda.is_available():
            sys.exit('guarded_step_profile.py times launches on the card: it needs a GPU, there is no fallback')
        print(json.dumps(kernels_leg(args.runs) if args.child == ['kernels'] else loop_leg(args.iters, args.warmup, args.child)))
        return
    if args.runs < 6:
        ap.error('--runs: at least six repetitions per leg')

    def child(tree, what):
        got = subprocess.run([sys.executable, os.path.abspath(__file__), '--tree', tree, '--iters', str(args.iters), '--warmup',
                              str(args.warmup), '--runs', str(args.runs), '--child'] + what, capture_output=True, text=True, timeout=300)
        if got.returncode:
            sys.exit(f'measurement of {tree} failed ({got.returncode}):\n{got.stderr[-2000:]}')
        return json.loads(got.stdout.strip().splitlines()[-1])

    doc = dict(kernels=child(ROOT, ['kernels']))
    print(json.dumps(doc['kernels']), flush=True)
    trees = ([('parent', args.parent, ['off'])] if args.parent else []) + [('branch', ROOT, ['off', 'on'])]
    rates = {}
    for run in range(args.runs):                           # the trees alternate, a fresh process each time
        for tag, tree, guards in trees:
            for line in child(tree, guards):
                rates.setdefault(f'{tag}_guard_{line["guard"]}', []).append(line)
                print(json.dumps(dict(run=run, tree=tag, **line)), flush=True)
    doc['loop'] = {k: dict(iters_per_s=spread([x['iters_per_s'] for x in v], 1), us_per_pair=spread([x['us_per_pair'] for x in v], 1),
                           runs=[x['iters_per_s'] for x in v], guard_stats=v[-1].get('guard_stats'))
                   for k, v in rates.items()}
    doc['loop_setup'] = dict(clip=CLIP, iters=args.iters, warmup=args.warmup, runs=args.runs,
                             parent='measured in the same job' if args.parent else 'not measured')
    print(json.dumps(doc['loop']), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)


if __name__ == '__main__':
    main()
