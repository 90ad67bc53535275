"""The per-lane walk state of gemm_kernel's im2col / permuted-weight / conv-gradient tile loaders (gemm.hip, OpWalk) against
the closed-form accessor off_of, on the host through mst_debug_gemm_walk: every lane of every 32-row tile walks [k0, k1) in
k-tiles of KD exactly as gemm_body does, and every element's predicates and offset must agree.  Zero mismatches, and the number
of elements walked is checked too, so a walk that compares nothing cannot pass."""
import ctypes as C

import pytest

from simutil import sim_native

OPK_IM2COL, OPK_PERMW, OPK_CONVGRAD = 3, 4, 5
KDS = (32, 64, 128)


def walk(kind, as_b, rows, K, k0, k1, kd, ld=0, pb=0, pc=0, oc=0):
    seen = C.c_int64(-1)
    bad = sim_native().lib.mst_debug_gemm_walk(kind, as_b, rows, K, k0, k1, kd, ld, pb, pc, oc, C.byref(seen))
    tiles, ktiles = (rows + 31) // 32, (k1 - k0 + kd - 1) // kd
    assert seen.value == tiles * ktiles * 32 * kd, (seen.value, tiles, ktiles)       # every element of every staged tile
    return bad


def k_ranges(K, kd):
    """k0 = 0 and every multiple of KD below K (a k-split's first k: not a multiple of 70 is the case that goes wrong), each
    with k1 = K and a k1 inside a tile"""
    for k0 in range(0, K, kd):
        yield k0, K
        inside = min(K, k0 + kd + kd // 2 + 3)      # the range's second tile is cut (the first where K ends before it)
        if inside != K:
            yield k0, inside
        yield k0, min(K, k0 + 5)                    # shorter than one k-tile


@pytest.mark.parametrize('kd', KDS)
@pytest.mark.parametrize('M', [8, 96, 2048])        # P = 1 (a partial row tile), 12, 256: octave 0 and octave 7 padding taps
def test_im2col_as_a(M, kd):
    for k0, k1 in k_ranges(700, kd):
        assert walk(OPK_IM2COL, 0, M, 700, k0, k1, kd) == 0, (k0, k1)


@pytest.mark.parametrize('kd', KDS)
@pytest.mark.parametrize('pb,pc,K,N', [(14, 5, 700, 57), (47, 2, 940, 64), (47, 2, 940, 45), (14, 5, 700, 33)])
def test_permuted_weight(pb, pc, K, N, kd):
    # (47, 2) with K = 940: the last 128-deep tile is 44 deep; N = 57 / 45 / 33 are no multiple of 32
    for k0, k1 in k_ranges(K, kd):
        assert walk(OPK_PERMW, 1, N, K, k0, k1, kd, ld=K, pb=pb, pc=pc) == 0, (k0, k1)


@pytest.mark.parametrize('kd', KDS)
def test_im2col_as_b_with_the_bias_column(kd):
    # the conv's weight gradient: N = 700 weight columns and the bias column (its offset is never loaded, its predicates are
    # used), k over (position, octave) rows; a k range shorter than one KD is what a k-split of a short clip gets
    for K in (8, 96, 2048):
        for k0, k1 in k_ranges(K, kd):
            assert walk(OPK_IM2COL, 1, 701, K, k0, k1, kd) == 0, (K, k0, k1)


@pytest.mark.parametrize('kd', KDS)
def test_conv_gradient_as_a(kd):
    for K in (8, 2048):
        for k0, k1 in k_ranges(K, kd):
            assert walk(OPK_CONVGRAD, 0, 57, K, k0, k1, kd, oc=57) == 0, (K, k0, k1)


def test_rejects_what_it_cannot_walk():
    lib = sim_native().lib
    assert lib.mst_debug_gemm_walk(OPK_PERMW, 1, 64, 700, 0, 700, 128, 700, 7, 10, 0, None) < 0      # not one of the model's permutations
    assert lib.mst_debug_gemm_walk(OPK_IM2COL, 0, 64, 700, 0, 700, 48, 0, 0, 0, 0, None) < 0         # no such k-tile depth
    assert lib.mst_debug_gemm_walk(OPK_IM2COL, 0, 64, 700, 0, 701, 128, 0, 0, 0, 0, None) < 0        # k1 beyond K
