"""Batched style transfer on the CPU: mst_clip_gather, mst_rolls_count / mst_rolls_compact and mst_style_sums (the product's kernel
source on the hipsim interpreter, the cases of tests/transfer_cases.py), their composition with the crops, the stage masks of
mst_forward, mst_clip_scatter and mst_roll_metrics at the C ABI, and the host side: style.metrics.style_cosines and
style.sparse.stitch_records."""
import numpy as np
import pytest
import torch

import simutil
import transfer_cases as tc


@pytest.mark.parametrize('case', tc.KERNEL_CASES, ids=[c.__name__[5:] for c in tc.KERNEL_CASES])
def test_kernels(case):
    case(simutil.sim_native(), 'cpu')


def test_composition_at_the_c_abi():
    tc.case_composition(simutil.sim_native(), 'cpu', K=3)


# ---- the host side
@pytest.mark.parametrize('key,crt,bars', [('pitched', (2, 6, 2), 2), ('unpitched', (2, 6, 2), 3), ('pitched', (3, 4, 1), 4),
                                          ('unpitched', (1, 5, 2), 1)])
def test_stitch_records_is_the_concatenation_along_the_bar_axis(key, crt, bars):
    """Windows of a synthetic song: stitch(...).to_numpy() is the dense rolls concatenated along the bar axis — a single window
    and cells in the last bar of the last channel included — and crop_bars is the slice of the dense roll."""
    from style.sparse import SparseRoll, crop_bars, sparsify, stitch_records
    from tools.synth import synth_clip
    x = synth_clip(11, *crt, True, density=.05)[key]
    x[0, -1, -1, -1, -1, -1] = torch.rand(x.shape[-1]) + .1               # the very last cell is live
    R = x.shape[2]
    assert R % bars == 0
    windows = [x[:, :, r0:r0 + bars].contiguous() for r0 in range(0, R, bars)]
    whole = stitch_records([sparsify(w, pin=False) for w in windows], bars)
    assert whole.shape == tuple(x.shape) and whole.count == sparsify(x, pin=False).count > len(windows)
    assert np.array_equal(whole.to_numpy().view(np.uint32), np.concatenate([w.numpy() for w in windows], axis=2).view(np.uint32))
    assert torch.equal(whole.packed, sparsify(x, pin=False).packed)       # sorted, and SparseRoll's own validation passed
    SparseRoll.from_packed(whole.packed, whole.shape)
    assert int(whole.cells[-1]) == whole.n_cells - 1
    for n in range(1, R + 1):
        cut = crop_bars(whole, n)
        assert cut.shape == tuple(x[:, :, :n].shape) and torch.equal(cut.packed, sparsify(x[:, :, :n], pin=False).packed), n
    for bad in (lambda: stitch_records([], bars), lambda: stitch_records([whole], bars + R), lambda: crop_bars(whole, 0),
                lambda: crop_bars(whole, R + 1), lambda: stitch_records([sparsify(windows[0], pin=False), sparsify(torch.zeros(1, x.shape[1], bars + 1, *x.shape[3:]), pin=False)], bars)):
        with pytest.raises(ValueError):
            bad()


def test_style_cosines():
    """The three cosines from mst_style_sums' words; NaN where a norm is 0."""
    from style.metrics import TransferResult, style_cosines
    rng = np.random.default_rng(4)
    x, y, z = rng.standard_normal((3, 5, 40))
    z[3] = 0.
    y[4] = x[4] * 2.5
    dot = lambda a, b: (a * b).sum(-1)
    sums = np.stack([dot(x, x), dot(y, y), dot(z, z), dot(x, y), dot(x, z), dot(y, z), np.full(5, 40.), np.zeros(5)], axis=-1)
    cos = style_cosines(torch.from_numpy(sums))
    assert cos.shape == (5, 3) and cos.dtype == np.float64
    want = lambda a, b: dot(a, b) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))
    with np.errstate(invalid='ignore'):
        ref = np.stack([want(x, y), want(x, z), want(y, z)], axis=-1)
    assert np.allclose(cos[:3], ref[:3], rtol=1e-14, atol=0) and np.isnan(cos[3]).tolist() == [False, True, True]
    assert abs(cos[4, 0] - 1) < 1e-15
    assert np.array_equal(style_cosines(sums[2]), cos[2]) and np.array_equal(TransferResult(*[None] * 5, torch.from_numpy(sums)).cosines, cos, equal_nan=True)
    with pytest.raises(ValueError):
        style_cosines(sums[:, :7])
