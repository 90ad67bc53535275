#!/usr/bin/env python3
"""Developer tool: the LSTM launches (W_hh transpose, recurrence forward / backward) of one training iteration at the default
and at wide style widths, and the one-clip iteration time of each model (HIP events, eager launches, bench clip shape).
Usage on the GPU box: python tools/lstm_widths_profile.py [C R T]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'music-style-transfer_amd')]
import numpy as np
import torch

from bench import CLIP, WIDTHS, KIND_NAMES, init_params
from tools.synth import synth_clip
from style import _native as nat

# style_size -> style encoder hidden size mean_size(bar, style): 256 -> 192 (default), 512 -> 320, 896 -> 512, 1920 -> 1024
STYLES = [256, 512, 896, 1920]
ITERS = 10

shape = dict(CLIP)
if len(sys.argv) >= 4:
    shape = dict(C=int(sys.argv[1]), R=int(sys.argv[2]), T=int(sys.argv[3]))
dev = torch.device('cuda:0')
native = nat.get()
clip = synth_clip(0, shape['C'], shape['R'], shape['T'], True)
xp, xu = clip['pitched'].contiguous().to(dev), clip['unpitched'].contiguous().to(dev)
for style in STYLES:
    widths = dict(WIDTHS, style=style)
    dims = nat.Dims(**shape, **widths, instr=51, n_instruments=41, has_unpitched=1, clips=1)
    flat, _ = init_params(native, dims)
    plan = native.plan(dims, dev)
    plan.set_inputs(mode=clip['mode'], bpm=clip['bpm'], instr=clip['instruments_features'], used=clip['used_instruments'],
                    bpm_target=120.)
    params = flat.to(dev)
    g = torch.zeros_like(params)
    for _ in range(2):
        plan.train_iteration(params, g, xp, xu)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        plan.train_iteration(params, g, xp, xu)
    e1.record()
    torch.cuda.synchronize()
    plan.check_status()
    iter_ms = e0.elapsed_time(e1) / ITERS
    lstm = []
    for bwd in (False, True):
        steps = plan.time_steps(7, bwd, params, g, xp, xu, reps=10)
        info = np.zeros((len(steps), 8), np.int32)
        native.lib.mst_plan_step_info(plan.handle, 7, int(bwd), info.ctypes.data)
        for (kind, ms, _, _), inf in zip(steps, info.tolist()):
            if kind in (3, 4, 11):
                B, S, H = inf[:3]
                lstm.append(dict(kernel=KIND_NAMES[kind], B=B, S=S, H=H, members=inf[4], us=round(ms * 1e3, 1),
                                 us_per_step=round(ms * 1e3 / S, 2) if S else None))
    print(json.dumps(dict(style=style, shape=shape, iteration_ms=round(iter_ms, 3), lstm_launches=lstm)))
