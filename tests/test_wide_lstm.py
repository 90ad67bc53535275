"""LSTM hidden sizes above 256 (csrc/lstm.hip wide flavour, up to 1024) on the CPU interpreter: every LSTM of the model at a
wide width against the oracle, batched and bar-tiled plans, launches that never mix flavour bands, and the one width rule that
mst_widths_supported and mst_plan_create share."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_cases as pc
from tools.synth import synth_clip
from simutil import make_dims, rel, sim_native
from style import _native as nat
from test_tiled import run_tiled

SMALL = pc.SMALL


def lstm_hidden_sizes(widths):
    """Hidden sizes of the seven LSTMs (style/model.py: mean_size of the constructor arguments)."""
    ms = lambda a, b, f=1.0: int(np.ceil((a + b) / 2 * f))
    return dict(beats=widths['beat'], bars=widths['bar'] // 2, style=ms(widths['bar'], widths['style']),
                si_beats=ms(10 * widths['rhythm'], widths['nrf'], .05), si_bars=widths['nrf'])


def lstm_steps(plan, kinds=(3, 11)):
    """LSTM launch steps of the forward (3 recurrence, 11 W_hh transpose): {B, S, H, multi, count, kind, level, chain}."""
    n = plan.lib.mst_plan_step_count(plan.handle, 7, 0)
    info = np.zeros((n, 8), np.int32)
    assert plan.lib.mst_plan_step_info(plan.handle, 7, 0, info.ctypes.data) == n
    return [tuple(r) for r in info.tolist() if r[5] in kinds]


@pytest.mark.parametrize('w,C_,R,T,unp,wide', [
    (dict(SMALL, style=600), 2, 3, 2, True, {'style': 303}),
    (dict(SMALL, bar=700), 2, 3, 2, True, {'bars': 350, 'style': 356}),
    (dict(SMALL, beat=300), 2, 2, 2, True, {'beats': 300}),
    (dict(SMALL, beat=300), 3, 2, 2, False, {'beats': 300}),
    (dict(SMALL, nrf=300), 2, 3, 2, True, {'si_bars': 300}),
    (dict(SMALL, style=2042), 1, 2, 2, True, {'style': 1024}),
])
def test_wide_lstms_match_the_oracle(w, C_, R, T, unp, wide):
    sizes = lstm_hidden_sizes(w)
    for k, h in wide.items():
        assert sizes[k] == h, (k, sizes[k], h)
    pc.oracle_case(sim_native(), 'cpu', w, C_, R, T, unp, density=0.05, check_bitwise=True)


def test_batched_wide_plan_equals_sequential_iterations():
    pc.batch_case(sim_native(), 'cpu', dict(SMALL, style=600), 2, 2, 2, True, 3)


def test_batched_wide_plan_on_the_mfma_gemm():
    # K >= 6 picks the 64x64 GEMM tiling on its own; forced here at a smaller K
    pc.batch_case(sim_native(), 'cpu', dict(SMALL, bar=700), 1, 2, 1, True, 2, gemm_tile=64)


def test_bar_tiled_wide_plan_equals_one_rank_plan():
    native = sim_native()
    w = dict(SMALL, style=600, bar=520)                # bars LSTMs 260, style encoder 560: the replicated bar-level chains
    Cn, R, T, unp = 2, 4, 1, True
    dims = make_dims(w, Cn, R, T, unp)
    flat, _, _ = pc.random_params(native, dims, 3)
    clip = synth_clip(21, Cn, R, T, unp, density=0.05)
    plan = nat.Plan(native, dims, 'cpu')
    pc.set_clip(plan, clip)
    g1 = torch.zeros_like(flat)
    l1 = torch.zeros(nat.N_LOSSES)
    a, b = pc.dev_clip(clip, 'cpu')
    plan.train_iteration(flat.clone(), g1, a, b, l1)
    gt, lt, plans, _ = run_tiled(native, 'cpu', w, Cn, R, T, unp, [(0, 2), (2, 2)], clip, flat)
    for l in lt:
        assert torch.allclose(l, l1, atol=2e-6, equal_nan=True), (l, l1)
    assert rel(gt.numpy(), g1.numpy()) < 2e-5
    for p in plans:
        assert rel(p.view('style').numpy(), plan.view('style').numpy()) < 1e-5


@pytest.mark.parametrize('w,groups', [
    (dict(SMALL, style=600, rhythm=600), [1, 1]),     # style encoder 303 (wide) | song-info beats LSTM 151 (L2)
    (dict(SMALL, bar=300, nrf=300), [1, 5]),          # song-info bars LSTM 300 (wide) | 4 bars LSTMs 150 + style encoder 156
])
def test_launches_never_mix_flavour_bands(w, groups):
    # the W_hh transposes of every LSTM sit at the first dependency level of the whole-model forward, where launches of one kernel
    # are merged across stages: the wide and the L2 flavour's stay apart
    native = sim_native()
    plan = nat.Plan(native, make_dims(w, 2, 3, 2, True), 'cpu')
    transposes = [s for s in lstm_steps(plan, (11,)) if s[6] == 0]
    assert sorted(s[4] for s in transposes) == groups, transposes
    pc.oracle_case(native, 'cpu', w, 2, 3, 2, True, density=0.05, check_bitwise=True)


@pytest.mark.parametrize('w,ok', [
    (dict(SMALL, style=2042), True),                  # style encoder H 1024
    (dict(SMALL, nrf=300), True),                     # song-info bars LSTM 300
    (dict(SMALL, style=2044), False),                 # style encoder H 1025
    (dict(SMALL, nrf=1025), False),                   # song-info bars LSTM 1025
    (dict(SMALL, rhythm=4099), False),                # song-info beats LSTM 1025
    (dict(SMALL, bar=2052), False),                   # channel encoders' bars LSTMs 1026
    (dict(SMALL, beat=1025), False),                  # channel encoders' beats LSTMs 1025
    (dict(SMALL, melody=6), False),                   # no note kernels for melody_size 6
])
def test_widths_supported_and_plan_create_agree(w, ok):
    native = sim_native()
    dims = make_dims(w, 1, 2, 1, True)
    want = 0 if ok else -2                             # MST_OK / MST_ERR_UNSUPPORTED
    assert native.lib.mst_widths_supported(C.byref(dims)) == want
    st = C.c_int32(7)
    handle = native.lib.mst_plan_create(C.byref(dims), C.byref(st))
    assert st.value == want and bool(handle) == ok
    if handle:
        native.lib.mst_plan_destroy(handle)
