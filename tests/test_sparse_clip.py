"""Sparse clip input on the CPU: mst_clip_scatter (the product's kernel source on the hipsim interpreter) and the host side
of style.data's SparseRoll / SparseClip.  The feature promises the same float32 bits as the dense path, so every comparison
is bit equality."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import simutil
from tools.synth import synth_clip

HERE = os.path.dirname(os.path.abspath(__file__))
MIDIS = sorted(glob.glob(os.path.join(HERE, 'golden', 'midi', '*.mid')))
SLICE = 2048            # floats of the destination one workgroup owns (SCAT_SLICE, csrc/loss_optim.hip)
NAN = float('nan')
assert len(MIDIS) == 10, 'the real-roll test leaves no example file out'


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def _same_bits(got, want):
    return got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _scatter(roll, out=None):
    """Densify on the interpreter into a NaN-poisoned destination."""
    out = torch.full(roll.shape, NAN) if out is None else out
    return roll.to_dense('cpu', out=out, native=simutil.sim_native())


def _rolls(clip):
    return [clip['pitched']] + ([clip['unpitched']] if clip['unpitched'] is not None else [])


@pytest.mark.parametrize('density', [0., .02, 1.])
@pytest.mark.parametrize('crt', [(2, 3, 2), (1, 5, 3)])
def test_scatter_of_sparsify_is_the_roll(crt, density):
    from style.data import sparsify
    for x in _rolls(synth_clip(3, *crt, True, density=density)):
        assert x.numel() % SLICE != 0                    # the last workgroup's slice is ragged
        roll = sparsify(x)
        assert roll.count == int((x != 0).any(-1).sum()) and roll.shape == tuple(x.shape)
        assert _same_bits(_scatter(roll), x)


def test_scatter_of_more_than_64k_records():
    """Above 65536 live records the workgroup-wide search of the kernel takes a third round."""
    from style.data import sparsify
    for x in _rolls(synth_clip(6, 1, 35, 4, True, density=1.)):
        roll = sparsify(x)
        assert roll.count == roll.n_cells > 1 << 16
        assert _same_bits(_scatter(roll), x)
    x = synth_clip(7, 1, 40, 4, True, density=.9)['unpitched']          # and with holes between the records
    roll = sparsify(x)
    assert 1 << 16 < roll.count < roll.n_cells
    assert _same_bits(_scatter(roll), x)


def test_scatter_into_a_destination_that_is_not_16_byte_aligned():
    from style.data import sparsify
    x = synth_clip(4, 1, 2, 1, True, density=.05)['pitched']
    roll = sparsify(x)
    for lead in (1, 2, 3):
        buf = torch.full((x.numel() + 8,), NAN)
        _scatter(roll, out=buf[lead:lead + x.numel()])
        assert _same_bits(buf[lead:lead + x.numel()].view(x.shape), x)
        assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + x.numel():]).all()      # nothing outside is touched


def test_negative_zero_and_float64_rolls_keep_their_float32_bits():
    from style.data import sparsify
    x = np.zeros((1, 1, 1, 1, 10, 56, 5))
    x[0, 0, 0, 0, 3, 7] = [-0., 0., 0., 0., 0.]           # all features compare equal to zero, one bit pattern is not
    x[0, 0, 0, 0, 9, 55] = [1 / 3, .1, 0., 1., 0.]        # not representable in float32
    roll = sparsify(x)
    assert roll.count == 2 and roll.feats.dtype == torch.float32
    want = torch.from_numpy(x.astype(np.float32))
    assert _same_bits(torch.from_numpy(roll.to_numpy()), want)
    assert _same_bits(_scatter(roll), want)


@pytest.mark.parametrize('path', MIDIS, ids=[os.path.basename(p) for p in MIDIS])
def test_scatter_of_the_real_rolls(path):
    from style.data import sparsify
    from style.style_transfer import get_model_input
    _, (_, pitched, _, _, unpitched) = get_model_input(path)
    for x in (pitched, unpitched):
        if x is None:
            continue
        roll = sparsify(x)
        assert 0 < roll.count < .02 * roll.n_cells
        assert _same_bits(_scatter(roll), torch.from_numpy(x.astype(np.float32)))


def _batched(rolls, capacity, garbage=False):
    """cells / feats / counts of several clips of one shape in the C ABI's batched layout."""
    nfeat = rolls[0].nfeat
    g = torch.Generator().manual_seed(7)
    cells = torch.zeros(len(rolls), capacity, dtype=torch.int32)
    feats = torch.zeros(len(rolls), capacity, nfeat)
    if garbage:                                           # whatever lies beyond a clip's count is ignored
        cells = torch.randint(-5, rolls[0].n_cells + 5, cells.shape, generator=g, dtype=torch.int32)
        feats = torch.rand(feats.shape, generator=g) + 1.
    for k, r in enumerate(rolls):
        cells[k, :r.count] = r.cells
        feats[k, :r.count] = r.feats
    return cells, feats, torch.tensor([r.count for r in rolls], dtype=torch.int32)


@pytest.mark.parametrize('garbage', [False, True])
def test_three_clips_in_one_call_with_their_own_counts(garbage):
    from style.data import sparsify
    xs = [synth_clip(10 + k, 2, 1, 2, True, density=d)['unpitched'] for k, d in enumerate((.03, 0., .2))]
    rolls = [sparsify(x) for x in xs]
    assert len({r.count for r in rolls}) == 3 and rolls[1].count == 0
    capacity = max(r.count for r in rolls) + 37
    cells, feats, counts = _batched(rolls, capacity, garbage)
    out = torch.full((3,) + tuple(xs[0].shape), NAN)
    simutil.sim_native().clip_scatter(cells, feats, counts, out, rolls[0].n_cells, 2, n_clips=3, capacity=capacity)
    assert _same_bits(out, torch.stack(xs))


def test_a_second_clip_leaves_no_cell_of_the_first():
    from style.data import sparsify
    a = synth_clip(20, 2, 2, 1, True, density=.5)['pitched']
    b = synth_clip(21, 2, 2, 1, True, density=.01)['pitched']
    out = torch.full(a.shape, NAN)
    _scatter(sparsify(a), out=out)
    assert _same_bits(out, a)
    _scatter(sparsify(b), out=out)
    assert _same_bits(out, b)


_OUT_OF_RANGE_CASE = '''
import sys
import numpy as np
import torch
sys.path[:0] = {paths!r}
import simutil
native = simutil.sim_native(asan={asan})
n_cells, nfeat = 1000, 5
# exactly-sized heap buffers: a store for the cells beyond the roll would land outside `out`
cells = torch.tensor([3, 999, 1000, 1001, 2 ** 31 - 1], dtype=torch.int32)
feats = torch.arange(1., 26.).reshape(5, 5).clone()
counts = torch.tensor([5], dtype=torch.int32)
out = torch.full((n_cells, nfeat), float('nan'))
native.clip_scatter(cells, feats, counts, out, n_cells, nfeat)
want = torch.zeros(n_cells, nfeat)
want[3], want[999] = feats[0], feats[1]
assert torch.equal(out, want), 'out-of-range cells must be skipped'
print('skipped ok')
'''


def _run_out_of_range_case(asan):
    env = dict(os.environ)
    if asan:
        rt = subprocess.run(['/opt/rocm/lib/llvm/bin/clang++', '-print-file-name=libclang_rt.asan-x86_64.so'],
                            capture_output=True, text=True, check=True).stdout.strip()
        assert os.path.exists(rt), rt
        # the ASan runtime only has to come first: whatever is preloaded already stays behind it
        old = env.get('LD_PRELOAD', '')
        env.update(LD_PRELOAD=rt + (':' + old if old else ''), ASAN_OPTIONS='detect_leaks=0')
    code = _OUT_OF_RANGE_CASE.format(paths=[HERE] + [p for p in sys.path if p], asan=asan)
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and 'skipped ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_out_of_range_cells_are_skipped():
    _run_out_of_range_case(asan=False)


def test_out_of_range_cells_are_skipped_under_asan():
    _run_out_of_range_case(asan=True)


# ---- host side
def test_to_numpy_round_trip_and_validation():
    from style.data import SparseRoll, sparsify
    x = synth_clip(5, 2, 2, 2, True, density=.1)['unpitched']
    roll = sparsify(x)
    assert roll.cells.dtype == torch.int32 and roll.feats.dtype == torch.float32 and roll.shape == tuple(x.shape)
    assert np.array_equal(roll.to_numpy().view(np.uint32), x.numpy().view(np.uint32))
    again = SparseRoll(roll.cells.numpy(), roll.feats.numpy(), roll.shape)
    assert np.array_equal(again.to_numpy(), x.numpy())
    f = np.ones((3, 2), np.float32)
    for bad in ([5, 4, 9], [4, 4, 9], [0, 1, 40], [-1, 2, 3]):           # unsorted, duplicate, out of range (both ends)
        with pytest.raises(ValueError):
            SparseRoll(np.array(bad, np.int32), f, (4, 10, 2))
    with pytest.raises(ValueError):
        SparseRoll(np.array([1, 2, 3], np.int32), np.ones((3, 5), np.float32), (4, 10, 2))    # feature count of the shape
    with pytest.raises(ValueError):
        SparseRoll(np.array([1], np.int32), np.ones((1, 3), np.float32), (4, 10, 3))          # neither pitched nor unpitched


def test_err_arg_cases():
    lib = simutil.sim_native().lib
    cells, feats, counts = torch.zeros(4, dtype=torch.int32), torch.zeros(4, 5), torch.ones(1, dtype=torch.int32)
    out = torch.zeros(10, 5)
    P = lambda t: t.data_ptr()
    call = lambda c, f, n, cap, clips, n_cells, nfeat, o: lib.mst_clip_scatter(c, f, n, cap, clips, n_cells, nfeat, o, None)
    assert call(P(cells), P(feats), P(counts), 4, 1, 10, 5, P(out)) == 0
    for args in ((None, P(feats), P(counts), 4, 1, 10, 5, P(out)), (P(cells), None, P(counts), 4, 1, 10, 5, P(out)),
                 (P(cells), P(feats), None, 4, 1, 10, 5, P(out)), (P(cells), P(feats), P(counts), 4, 1, 10, 5, None),
                 (P(cells), P(feats), P(counts), 4, 1, 10, 3, P(out)), (P(cells), P(feats), P(counts), 4, 1, 10, 0, P(out)),
                 (P(cells), P(feats), P(counts), 4, 1, 2 ** 31, 5, P(out)), (P(cells), P(feats), P(counts), 4, 1, 0, 5, P(out)),
                 (P(cells), P(feats), P(counts), 4, 0, 10, 5, P(out)), (P(cells), P(feats), P(counts), -1, 1, 10, 5, P(out))):
        assert call(*args) == -1, args                    # MST_ERR_ARG
    assert torch.equal(out, torch.zeros(10, 5))


def _song(seed=0, C=2, R=7, unpitched=True, silent_unpitched=False):
    rng = np.random.default_rng(seed)
    roll = lambda shape: rng.random(shape) * (rng.random(shape[:-1] + (1,)) < .03)
    u = roll((1, R, 4, 10, 47, 2)) if unpitched else None
    if silent_unpitched:
        u[:] = 0.
    info = dict(bpm=97, scale=dict(mode='major' if seed % 2 else 'minor'))
    feats = np.zeros((C, 51))
    feats[np.arange(C), np.arange(C)] = 1.
    return 'song', (info, roll((C, R, 4, 10, 56, 5)), feats, list(range(C)), u)


@pytest.mark.parametrize('max_n_bars', [None, 5, 50])
def test_prepare_input_sparse_matches_prepare_input(max_n_bars):
    from style.data import prepare_input, prepare_input_sparse, SparseClip, SparseRoll
    for song in (_song(1), _song(2, C=1, unpitched=False)):
        dense = [None if t is None else t.cpu() for t in prepare_input(song, max_n_bars)]
        clip = prepare_input_sparse(song, max_n_bars)
        assert isinstance(clip, SparseClip) and clip.bpm_target == 97
        items = list(clip)
        assert len(items) == 5 and isinstance(items[2], SparseRoll)
        for i in (0, 1, 3):
            assert _same_bits(items[i], dense[i])
        for i in (2, 4):
            if dense[i] is None:
                assert items[i] is None
                continue
            assert items[i].shape == tuple(dense[i].shape)              # the cut to max_n_bars included
            assert _same_bits(torch.from_numpy(items[i].to_numpy()), dense[i])
            assert _same_bits(_scatter(items[i]), dense[i])
        via_kernel = clip.to_dense('cpu', native=simutil.sim_native())
        assert all((a is None and b is None) or _same_bits(a, b) for a, b in zip(via_kernel, dense))


def test_save_load_round_trip(tmp_path):
    from style.data import prepare_input_sparse, SparseClip
    for k, song in enumerate((_song(3), _song(4, unpitched=False))):
        clip = prepare_input_sparse(song, 6)
        path = str(tmp_path / f'clip{k}.npz')
        clip.save(path)
        assert os.path.getsize(path) < 200_000
        back = SparseClip.load(path)
        assert back.bpm_target == clip.bpm_target and type(back.bpm_target) is type(clip.bpm_target)
        for a, b in zip(clip, back):
            if a is None or b is None:
                assert a is None and b is None
            elif torch.is_tensor(a):
                assert _same_bits(a, b)
            else:
                assert a.shape == b.shape and torch.equal(a.cells, b.cells) and _same_bits(a.feats, b.feats)


def test_drop_silent_on_the_records_agrees_with_the_rolls():
    from style.data import prepare_input_sparse
    from style.train import drop_silent, iter_sparse
    songs = [_song(5), _song(6, silent_unpitched=True), _song(7, unpitched=False)]
    silent = _song(8)
    silent[1][1][:] = 0.
    songs.append(silent)
    got = list(iter_sparse(iter(songs)))
    for song, clip in zip(songs, got):
        kept, cap = drop_silent(song)
        if kept is None:
            assert clip is None
            continue
        assert (clip.unpitched_channels is None) == (kept[1][4] is None)
        assert clip.pitched_channels.shape[2] == min(cap, song[1][1].shape[1])
    assert got[3] is None and got[1].unpitched_channels is None and got[0].unpitched_channels is not None
