"""Width lattice for the batched Linear and convolution kernels (csrc/lin.hip, csrc/conv.hip), shared by the CPU-interpreter
tests and the -m gpu tests.  parity_cases.FULL and SMALL fix the shape of every Linear through mst_sizes, so the plans of the
other test files reach 18 of the 92 (kernel family x width residue) cells of lin.hip, never a K = 1 or 3 (mod 4), and conv.hip
at OC = 57 and 29 only.  LATTICE is a list of width sets, found by scanning plan creation on the interpreter, whose lin.hip
steps cover every cell and whose row counts and convolution widths sit on the kernels' edges; run() puts each of them against
the float64 oracle (precision_cases.precise_case: no tolerance of its own)."""
import numpy as np
import torch

import parity_cases as pc
import precision_cases as pr
from simutil import make_dims
from style import _native as nat

K_CONV_P, K_CONV_F, K_CONV_W, K_LIN_F, K_LIN_A, K_LIN_W = 26, 27, 28, 29, 30, 31      # step kinds (plan.hip: "the values are ABI")
LN16_JMAX = 320

FWD_FAMILIES = ('lin16_fwd', 'rows<4,1,0>', 'rows<2,2,0>')
DW_FAMILIES = ('lin16_dw', 'dw<1,4>', 'dw<2,2>')
DX_FAMILIES = ('rows<4,1,1>', 'rows<2,2,1>')
ALL_CELLS = frozenset([('fwd', f, k) for f in FWD_FAMILIES for k in range(4)] +
                      [('dw', f, n, k) for f in DW_FAMILIES for n in range(4) for k in range(4)] +
                      [('dx', f, n, k) for f in DX_FAMILIES for n in range(4) for k in range(4)])
assert len(ALL_CELLS) == 92
# cells that no supported width set with every LSTM hidden size <= 256 reaches: (cell, reason).  None: a random scan of 2500
# supported width sets at (C, R, T) = (2, 4, 4) reaches all 92.
UNREACHABLE = ()


def step_rows(plan, backward, mask=7):
    n = plan.lib.mst_plan_step_count(plan.handle, mask, int(backward))
    info = np.zeros((n, 8), np.int32)
    assert plan.lib.mst_plan_step_info(plan.handle, mask, int(backward), info.ctypes.data) == n
    return info.tolist()


def lin_steps(plan):
    """{(kind, rows, N, K)} of the lin.hip steps of the whole-model forward and backward passes"""
    return {(r[5], r[0], r[1], r[2]) for b in (False, True) for r in step_rows(plan, b) if r[5] in (K_LIN_F, K_LIN_A, K_LIN_W)}


def step_kinds(plan):
    return {r[5] for b in (False, True) for r in step_rows(plan, b)}


def lin_cells(plan):
    """The cells a plan's lin.hip steps fall into: (pass, kernel family, residues mod 4 of the widths whose ragged end the
    kernel handles).  The family is the kernel that launch_lin_fwd / launch_lin_dx / launch_lin_dw (csrc/lin.hip) pick:
      lin_is16: N <= 16 and K + 1 <= LN16_JMAX -> lin16_fwd_kernel / lin16_dw_kernel (the input gradient has no lin16 kernel)
      forward, weight gradient: N <= 64 -> lin_rows_kernel<4,1,0> / lin_dw_kernel<1,4>, else <2,2,0> / <2,2>
      input gradient: K <= 64 -> lin_rows_kernel<4,1,1>, else <2,2,1>
    The forward reduces over K only (ln_ld4 / ln_fix4 on K-long rows); the two gradients load rows of both N and K elements."""
    cells = set()
    for kind, rows, N, K in lin_steps(plan):
        is16 = N <= 16 and K + 1 <= LN16_JMAX
        if kind == K_LIN_F:
            cells.add(('fwd', FWD_FAMILIES[0 if is16 else 1 if N <= 64 else 2], K % 4))
        elif kind == K_LIN_W:
            cells.add(('dw', DW_FAMILIES[0 if is16 else 1 if N <= 64 else 2], N % 4, K % 4))
        else:
            cells.add(('dx', DX_FAMILIES[0 if K <= 64 else 1], N % 4, K % 4))
    return cells


FORCED = dict(gemm_tile=64, dense_flavour=2)       # the 64x64 tiling with every eligible Linear (rows >= 32) on lin.hip
# (widths, C, R, T, clips, options of precise_case: the plan options and `seed` of the parameter draw).  Every LSTM hidden size
# (beat, bar / 2, (bar + style) / 2, ...) is <= 256.  The reference condition of precise_case (fp32 oracle within TOL / 8 of
# float64 on every tensor) depends on the host that evaluates the oracle: each seed is the one of 0..7 whose worst tensor is
# smallest over two hosts (an Intel and an AMD CPU, both on MKL), at most 3.3e-6 there against the bound 1.25e-5.
# No entry has melody 4: on the AMD host the fp32 oracle's melody_encoder.linear.weight is 2e-5 ... 1e-4 from float64 for every
# seed at melody 4 and widths like these (the cancellation precision_cases._one_thread describes), and at most 3e-6 at 8 / 12 / 16.
LATTICE = [
    # --- conv.hip: OC = ceil((50 + beat) / 2).  OC = 64 is its limit, 33 / 32 cross its 32-column block, 65 leaves it.
    # P = C R T = 8: the minimum of conv.hip, ragged against the 32 positions of a tile
    (dict(beat=78, bar=26, nrf=2, style=57, melody=8, rhythm=53), 2, 2, 2, 2, dict(FORCED)),            # 0: OC = 64
    # rhythm 32: pitched_rhythm_encoder.channels_linear is 280 -> 16, the widest lin16 shape
    (dict(beat=16, bar=110, nrf=10, style=196, melody=8, rhythm=32), 2, 4, 4, 2, dict(FORCED, seed=2)), # 1: OC = 33
    (dict(beat=14, bar=368, nrf=8, style=27, melody=16, rhythm=13), 2, 4, 4, 2, dict(FORCED, seed=5)),  # 2: OC = 32
    # rhythm 59: channels_linear is 280 -> 17, the first N past lin16
    (dict(beat=79, bar=264, nrf=7, style=139, melody=12, rhythm=59), 2, 4, 4, 2, dict(FORCED, seed=2)), # 3: OC = 65
    # --- 35 rows per clip, 3 clips: every 32-row k-tile of a weight gradient and every row tile of a forward straddles a clip
    (dict(beat=120, bar=194, nrf=11, style=63, melody=12, rhythm=61), 5, 7, 1, 3, dict(FORCED, seed=1)),# 4
    # --- one clip at (2, 4, 4): Linears of exactly 32 rows, the routing gate.  Entry 5 keeps to small widths: with entry 0 it
    # is the subset that the interpreter runs numerically (tests/test_dense_lattice.py)
    (dict(beat=45, bar=46, nrf=4, style=157, melody=8, rhythm=55), 2, 4, 4, 1, dict(FORCED)),           # 5
    (dict(beat=125, bar=236, nrf=4, style=242, melody=16, rhythm=44), 2, 4, 4, 1, dict(FORCED, seed=4)),# 6
    (dict(beat=142, bar=310, nrf=10, style=6, melody=12, rhythm=14), 2, 4, 4, 1, dict(FORCED, seed=4)), # 7
    (dict(beat=190, bar=128, nrf=9, style=104, melody=12, rhythm=15), 2, 4, 4, 1, dict(FORCED, seed=3)),# 8
    (dict(beat=211, bar=172, nrf=11, style=149, melody=8, rhythm=35), 2, 4, 4, 1, dict(FORCED, seed=6)),# 9
    # --- default routing on the same ragged widths: one clip on the 32x32 split-K tiling (accessor GEMM only), and 6 clips,
    # which pick the 64x64 tiling, conv.hip and the default lin.hip rule on their own
    (dict(beat=45, bar=46, nrf=4, style=157, melody=8, rhythm=55), 2, 4, 4, 1, dict()),                # 10
    (dict(beat=78, bar=26, nrf=2, style=57, melody=8, rhythm=53), 2, 2, 2, 6, dict()),                 # 11
]
FORCED_ENTRIES = [i for i, e in enumerate(LATTICE) if e[5].get('dense_flavour') == 2 and e[5].get('gemm_tile') == 64]
DENSITY = 0.05


def tag(i):
    w, C, R, T, clips, opts = LATTICE[i]
    return f'lattice {i}: ' + ' '.join(f'{k} {v}' for k, v in w.items()) + f' C{C} R{R} T{T} K{clips} {opts}'


def make_plan(native, device, entry):
    w, C, R, T, clips, opts = entry
    return nat.Plan(native, make_dims(w, C, R, T, True, clips=clips), device,
                    **{k: v for k, v in opts.items() if k != 'seed'})


def two_runs(native, device, entry):
    """The entry's train iteration twice on one plan (the inputs of precise_case, NaN-poisoned arenas before each run): gradients,
    losses and the activations of every clip agree bit for bit (fixed summation order everywhere)."""
    w, C, R, T, clips, opts = entry
    o = pr.oracle_runs(native, w, C, R, T, True, clips, DENSITY, 1.0, opts.get('seed', 0))
    plan = make_plan(native, device, entry)
    for k, clip in enumerate(o['clips']):
        plan.set_inputs(mode=clip['mode'], bpm=clip['bpm'], instr=clip['instruments_features'], used=clip['used_instruments'],
                        bpm_target=float(clip['bpm_int']), clip=k)
    xp = torch.cat([c['pitched'] for c in o['clips']]).contiguous().to(device)
    xu = torch.cat([c['unpitched'] for c in o['clips']]).contiguous().to(device)
    params = o['flat'].to(device)
    slots = ('style', 'melody', 'rhythm', 'pitched_pred', 'unpitched_pred')
    runs = []
    for _ in range(2):
        g, losses = torch.zeros_like(params), torch.zeros(clips, nat.N_LOSSES, device=device)
        pc.poison(plan)
        plan.train_iteration(params, g, xp, xu, losses)
        runs.append((g, losses.nan_to_num(-1.), {(s, k): plan.view(s, clip=k).clone() for s in slots for k in range(clips)}))
    (g1, l1, a1), (g2, l2, a2) = runs
    assert torch.equal(g2, g1), ('second run: gradients differ', float((g2 - g1).abs().max()))
    assert torch.equal(l2, l1), 'second run: losses differ'
    for key in a1:
        assert torch.equal(a2[key], a1[key]), ('second run: activation differs', key)


def run(native, device, entry, tag=None):
    """precise_case on the entry (every parameter gradient tensor, activation and stage-boundary gradient within pc.TOL of
    float64, the admission conditions asserted inside), then two_runs, and for a batched entry parity_cases.batch_case:
    bit-equality with the one-clip plan on the same tiling."""
    w, C, R, T, clips, opts = entry
    table = pr.precise_case(native, device, w, C, R, T, True, K=clips, density=DENSITY, tag=tag, **opts)
    two_runs(native, device, entry)
    if clips > 1:
        plan_opts = {k: v for k, v in opts.items() if k != 'seed'}
        pc.batch_case(native, device, w, C, R, T, True, clips, seed=opts.get('seed', 0), density=DENSITY, check_oracle=False, **plan_opts)
    return table
