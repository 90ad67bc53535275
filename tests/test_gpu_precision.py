"""-m gpu: the hipcc/gfx950 build on a real MI355X against the oracle evaluated in FLOAT64 (precision_cases): the list of
tests/test_sim_precision.py, plus the kernels that only the GPU build or larger widths select, each at the smallest shape an
existing -m gpu test uses for it.  On the card the exponentials are the hardware's and the GEMMs run on MFMA."""
import pytest
import torch

import parity_cases as pc
import precision_cases as pr

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SMALL, FULL = pc.SMALL, pc.FULL


@pytest.fixture(scope='module')
def native():
    from style import _native as nat
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return nat.get()       # raises if libmst_amd.so is missing: no fallback


def run(native, tag, *a, **kw):
    pr.precise_case(native, DEV, *a, tag=tag, **kw)


@pytest.mark.parametrize('C,R,T,unp', [(1, 1, 1, True), (3, 2, 3, False), (2, 5, 1, True), (3, 3, 2, True)])
def test_every_gradient_tensor_small_widths(native, C, R, T, unp):
    run(native, f'SMALL C{C} R{R} T{T} unp={unp}', SMALL, C, R, T, unp, density=0.05)


def test_lstm_gates_away_from_zero_small_widths(native):
    run(native, 'SMALL C3 R2 T3 lstm x 8', SMALL, 3, 2, 3, True, density=0.3, lstm_scale=8)


@pytest.mark.parametrize('tile', [None, 64])
def test_three_clip_plan_small_widths(native, tile):
    run(native, f'SMALL C2 R2 T1 K3 gemm_tile={tile}', SMALL, 2, 2, 1, True, K=3, density=0.03, gemm_tile=tile)


def test_every_gradient_tensor_full_widths(native):
    run(native, 'FULL C2 R2 T2', FULL, 2, 2, 2, True, density=0.03)


def test_lstm_gates_away_from_zero_full_widths(native):
    run(native, 'FULL C2 R2 T2 lstm x 6', FULL, 2, 2, 2, True, density=0.1, lstm_scale=6)


def test_large_linear_kernels_full_widths(native):
    run(native, 'FULL C2 R3 T2 gemm_tile=64 dense_flavour=2', FULL, 2, 3, 2, True, density=0.03, gemm_tile=64, dense_flavour=2)


def test_single_clip_on_the_mfma_gemm(native, monkeypatch):
    monkeypatch.setenv('MST_GEMM', 'mfma')
    run(native, 'FULL C2 R2 T2 MST_GEMM=mfma', FULL, 2, 2, 2, True, density=0.03)


@pytest.mark.parametrize('opts', [dict(gemm_tile=None), dict(gemm_tile=64), dict(gemm_tile=64, dense_flavour=2)],
                         ids=['tile-default', 'tile-64', 'tile-64-dense-2'])
def test_five_clip_plan_full_widths(native, opts):
    run(native, f'FULL C3 R4 T2 K5 {opts}', FULL, 3, 4, 2, True, K=5, density=0.03, **opts)


# seeds of the (2, 8, 4) cases: with the parameter draw of seed 0 the fp32 yardstick misses the reference condition for style 512
# (2.1e-5) and for the LSTM parameters x 6 (3.5e-5), and meets it by 1.6 % unscaled (1.23e-5); the seeds below are at 6.1e-6 or
# better under two different host BLAS paths (DESIGN.md 4.1 has the scan)
@pytest.mark.parametrize('W', [12, 16])
def test_melody_widths(native, W):
    run(native, f'melody {W} C2 R8 T4', dict(FULL, melody=W), 2, 8, 4, True, density=0.02)


@pytest.mark.parametrize('w,C,R,T,seed', [(dict(FULL, style=512), 2, 8, 4, 8), (dict(FULL, beat=320), 4, 4, 2, 0)], ids=['style-512', 'beat-320'])
def test_wide_lstms(native, w, C, R, T, seed):
    tag = ' '.join(f'{k} {v}' for k, v in w.items() if FULL[k] != v)
    run(native, f'{tag} C{C} R{R} T{T} seed {seed}', w, C, R, T, True, density=0.02, seed=seed)


@pytest.mark.parametrize('scale,density,seed', [(1.0, 0.02, 10), (6.0, 0.1, 18)], ids=['unscaled', 'lstm-x6'])
@pytest.mark.parametrize('flavour', [None, 1], ids=['flavour-default', 'flavour-1'])
def test_lstm_flavours(native, flavour, scale, density, seed):
    # default: the H = 192 style LSTM runs on 12 workgroups per sequence, exchanging h_t / dz_t over the 8 bars;
    # lstm_flavour = 1 keeps it on one workgroup
    run(native, f'FULL C2 R8 T4 lstm_flavour={flavour} lstm x {scale:g} seed {seed}', FULL, 2, 8, 4, True, density=density,
        lstm_scale=scale, seed=seed, lstm_flavour=flavour)


def test_loss_kernels_at_their_edges(native):
    pr.loss_edge_case(native, DEV)


def test_adam_across_two_steplr_boundaries(native):
    pr.adam_schedule_case(native, DEV)
