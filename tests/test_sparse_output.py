"""Sparse clip output on the CPU: mst_roll_count / mst_roll_compact (the product's kernel source on the hipsim interpreter),
style.data.compact, SparseRoll.from_packed and the host decode from note records (ChannelConverter.records2qchannel).  The
feature promises the records of the dense path bit for bit, so every comparison is bit equality.  Destinations are exactly
sized and sentinel-filled (cells -7, feats NaN): a store outside the promised range lands on a sentinel or outside the buffer."""
import glob
import os

import numpy as np
import pytest
import torch

import simutil
from tools.synth import synth_clip

HERE = os.path.dirname(os.path.abspath(__file__))
MIDIS = sorted(glob.glob(os.path.join(HERE, 'golden', 'midi', '*.mid')))
S = 1024                # cells of the roll one workgroup owns (ROLL_SLICE, csrc/loss_optim.hip)
NONZERO, HARD = 0, 1    # MST_ROLL_NONZERO, MST_ROLL_HARD
NAN = float('nan')
assert len(MIDIS) == 10, 'the real-roll test leaves no example file out'


def _native():
    native = simutil.sim_native()
    assert native.roll_slices(S) == 1 and native.roll_slices(S + 1) == 2, 'S above is not the kernels\' slice'
    return native


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def _same_bits(got, want):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    return got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _raw(x, mode, capacity=None, guard=0):
    """count + compact through the C ABI into sentinel-filled destinations of `capacity` records (default: the total) with
    `guard` spare elements on each side.  Returns ws, the cells buffer, the feats buffer (guards included)."""
    native = _native()
    nfeat = x.shape[-1]
    n_cells = x.numel() // nfeat
    SL = native.roll_slices(n_cells)
    ws = torch.full((SL + 1,), -7, dtype=torch.int32)
    native.roll_count(x, n_cells, nfeat, mode, ws)
    total = int(ws[-1])
    capacity = total if capacity is None else capacity
    cells = torch.full((capacity + 2 * guard,), -7, dtype=torch.int32)
    feats = torch.full(((capacity + 2 * guard) * nfeat,), NAN)
    if cells.numel() == 0:                                       # (an empty tensor has no address to hand over)
        return ws, cells, feats
    native.roll_compact(x, n_cells, nfeat, mode, ws, capacity, cells.data_ptr() + 4 * guard, feats.data_ptr() + 4 * guard * nfeat)
    return ws, cells, feats


def _want_nonzero(x):
    nfeat = x.shape[-1]
    flat = x.contiguous().view(-1, nfeat)
    idx = np.flatnonzero(flat.view(torch.int32).numpy().any(axis=1))
    return torch.from_numpy(idx.astype(np.int32)), flat[torch.from_numpy(idx)]


def _want_hard(x, out=None):
    """Records of the dense hard roll: the cells with a non-zero velocity, with the hard features."""
    from oracle import style_oracle as so
    out = so.hard_output(x.clone()) if out is None else torch.as_tensor(out)
    flat = out.contiguous().view(-1, out.shape[-1])
    idx = np.flatnonzero(flat[:, 1].numpy())
    return torch.from_numpy(idx.astype(np.int32)), flat[torch.from_numpy(idx)]


def _is(roll, want, shape):
    cells, feats = want
    return roll.shape == tuple(shape) and roll.count == len(cells) and torch.equal(roll.cells, cells) and _same_bits(roll.feats, feats)


def _rolls(clip):
    return [clip['pitched']] + ([clip['unpitched']] if clip['unpitched'] is not None else [])


def _compact(x, mode):
    from style.data import compact
    return compact(x, mode, native=_native())


# ---- 1
@pytest.mark.parametrize('density', [0., .02, 1.])
@pytest.mark.parametrize('crt', [(2, 3, 2), (1, 5, 3)])
def test_compact_is_the_inverse_of_the_scatter(crt, density):
    from style.data import sparsify
    for x in _rolls(synth_clip(3, *crt, True, density=density)):
        n_cells = x.numel() // x.shape[-1]
        assert n_cells % S != 0 and _native().roll_slices(n_cells) >= 3      # several slices, the last one ragged
        roll, want = _compact(x, 'nonzero'), sparsify(x)
        assert roll.shape == tuple(x.shape) and roll.count == want.count
        assert torch.equal(roll.cells, want.cells) and _same_bits(roll.feats, want.feats)
        assert torch.equal(roll.packed, want.packed)
        if density in (0., 1.):
            assert roll.count == int(density) * n_cells
        back = roll.to_dense('cpu', out=torch.full(x.shape, NAN), native=_native())
        assert _same_bits(back, x)


# ---- 2
@pytest.mark.parametrize('mode', ['nonzero', 'hard'])
def test_one_ragged_slice_only(mode):
    x = synth_clip(8, 1, 1, 1, True, density=.1)['unpitched']
    assert tuple(x.shape) == (1, 1, 1, 1, 10, 47, 2) and x.numel() // 2 == 470 < S and _native().roll_slices(470) == 1
    x[0, 0, 0, 0, 9, 46] = torch.tensor([.5, .7])                # the very last cell is live
    want = _want_nonzero(x) if mode == 'nonzero' else _want_hard(x)
    assert 0 < len(want[0]) < 470 and int(want[0][-1]) == 469
    assert _is(_compact(x, mode), want, x.shape)


# ---- 3
def test_empty_slices_between_live_ones():
    x = torch.zeros(1, 2, 3, 2, 10, 56, 5)
    n = x.numel() // 5
    SL = _native().roll_slices(n)
    assert n == 6720 and SL == 7 and (SL - 1) * S < n - 4
    live = [0, S - 1, S, (SL - 1) * S, (SL - 1) * S + 77, n - 3, n - 1]   # slices 2 .. SL - 2 are empty
    g = torch.Generator().manual_seed(1)
    x.view(-1, 5)[live] = torch.rand(len(live), 5, generator=g) + .2
    ws, cells, feats = _raw(x, NONZERO)
    per_slice = np.bincount(np.asarray(live) // S, minlength=SL)
    assert list(per_slice) == [2, 1, 0, 0, 0, 0, 4]
    assert ws.tolist() == [0] + list(np.cumsum(per_slice))       # the exclusive prefix, then the total
    assert cells.tolist() == live and _same_bits(feats.view(-1, 5), x.view(-1, 5)[live])
    assert _is(_compact(x, 'hard'), _want_hard(x), x.shape)


# ---- 4
def test_negative_zero_and_nan():
    x = torch.zeros(1, 1, 1, 3, 10, 56, 5)
    cell = lambda *idx: int(np.ravel_multi_index(idx, x.shape[:-1]))
    x[0, 0, 0, 0, 3, 7] = torch.tensor([-0., 0., 0., 0., 0.])    # compares equal to zero, one bit pattern is not
    x[0, 0, 0, 1, 2, 5] = torch.tensor([1., NAN, 0., 1., 0.])    # NaN velocity: hard_output zeroes it
    x[0, 0, 0, 2, 9, 55] = torch.tensor([2., .5, 0., .3, .2])
    assert x.numel() // 5 > S
    roll = _compact(x, 'nonzero')
    assert roll.cells.tolist() == [cell(0, 0, 0, 0, 3, 7), cell(0, 0, 0, 1, 2, 5), cell(0, 0, 0, 2, 9, 55)]
    assert _same_bits(roll.feats, x.view(-1, 5)[roll.cells.long()])
    hard = _compact(x, 'hard')
    assert hard.cells.tolist() == [cell(0, 0, 0, 2, 9, 55)]
    assert _same_bits(hard.feats, torch.tensor([[2., .5, 0., 1., 0.]]))       # (mst_hard_output's `v > .01f ? v : 0` zeroes a NaN)


# ---- 5
@pytest.mark.parametrize('name,out_name,live', [('hard/x_in', 'hard/x_out', (1115, 2240)), ('hard/u_in', 'hard/u_out', (452, 940)),
                                                ('swap/pitched', 'swap/hard_pitched', (3360, 3360)),
                                                ('swap/unpitched', 'swap/hard_unpitched', (2820, 2820))])
def test_hard_mode_against_the_reference_fixture(name, out_name, live):
    with np.load(os.path.join(simutil.GOLDEN, 'inference_small.npz')) as z:
        x, out = torch.from_numpy(z[name].copy()), torch.from_numpy(z[out_name].copy())
    before = x.clone()
    want = _want_hard(None, out)
    assert (len(want[0]), x.numel() // x.shape[-1]) == live
    assert _is(_compact(x, 'hard'), want, x.shape)
    assert _same_bits(x, before)                                 # unlike hard_output, the input keeps its velocities


# ---- 6
@pytest.mark.parametrize('path', MIDIS, ids=[os.path.basename(p) for p in MIDIS])
def test_hard_mode_on_the_real_rolls(path):
    from style.style_transfer import get_model_input
    _, (_, pitched, _, _, unpitched) = get_model_input(path)
    for roll in (pitched, unpitched):
        if roll is None:
            continue
        x = torch.from_numpy(roll.astype(np.float32))
        want = _want_hard(x)
        got = _compact(x, 'hard')
        assert 0 < got.count < .02 * got.n_cells and _is(got, want, x.shape)
        if 'Heroic' in os.path.basename(path) and roll is pitched:
            # the threshold drops six notes: a kernel that tests `!= 0` fails here
            assert got.count == 6072 and int((x[..., 1] != 0).sum()) == 6078


def test_the_heroic_polonaise_is_among_the_real_rolls():
    assert sum('Heroic' in os.path.basename(p) for p in MIDIS) == 1


# ---- 7
@pytest.mark.parametrize('mode', [NONZERO, HARD])
@pytest.mark.parametrize('nfeat', [5, 2])
def test_unaligned_source_and_guarded_destination(nfeat, mode):
    x = synth_clip(4, 1, 2, 2, True, density=.05)['pitched' if nfeat == 5 else 'unpitched'].contiguous()
    assert x.numel() // nfeat > S and (x.numel() // nfeat) % S
    ws0, cells0, feats0 = _raw(x, mode)
    assert 0 < int(ws0[-1]) == cells0.numel()
    want = _want_nonzero(x) if mode == NONZERO else _want_hard(x)
    assert torch.equal(cells0, want[0]) and _same_bits(feats0.view(-1, nfeat), want[1])
    for lead in (1, 2, 3):
        buf = torch.full((x.numel() + 8,), NAN)
        assert buf.data_ptr() % 16 == 0
        buf[lead:lead + x.numel()] = x.reshape(-1)
        view = buf[lead:lead + x.numel()].view(x.shape)
        assert view.data_ptr() % 16 == 4 * lead
        ws, cells, feats = _raw(view, mode, guard=8)
        assert torch.equal(ws, ws0)
        assert torch.equal(cells[8:-8], cells0) and _same_bits(feats[8 * nfeat:-8 * nfeat], feats0)
        assert (cells[:8] == -7).all() and (cells[-8:] == -7).all()                  # nothing outside the destination
        assert torch.isnan(feats[:8 * nfeat]).all() and torch.isnan(feats[-8 * nfeat:]).all()


# ---- 8
def test_capacity_below_the_count():
    x = synth_clip(9, 2, 3, 2, True, density=.02)['pitched']
    ws0, cells0, feats0 = _raw(x, NONZERO)
    total = int(ws0[-1])
    assert total > 40 and int(ws0[-2]) < total - 5 < total       # the cut falls inside the last slice
    for capacity in (total - 5, int(ws0[2]), 0):                 # inside a slice, on a slice boundary, nothing at all
        ws, cells, feats = _raw(x, NONZERO, capacity=capacity, guard=8)
        assert int(ws[-1]) == total and torch.equal(ws, ws0)     # the workspace still holds the true total
        assert torch.equal(cells[8:8 + capacity], cells0[:capacity]) and _same_bits(feats[40:40 + 5 * capacity], feats0[:5 * capacity])
        assert (cells[:8] == -7).all() and (cells[8 + capacity:] == -7).all()
        assert torch.isnan(feats[:40]).all() and torch.isnan(feats[40 + 5 * capacity:]).all()


# ---- 9
def test_err_arg_cases():
    lib = _native().lib
    x = torch.rand(10, 5) + .5
    ws = torch.full((2,), -7, dtype=torch.int32)
    cells, feats = torch.full((10,), -7, dtype=torch.int32), torch.full((50,), NAN)
    P = lambda t: t.data_ptr()
    assert lib.mst_roll_slices(0) <= 0 and lib.mst_roll_slices(-3) <= 0 and lib.mst_roll_slices(2 ** 31) <= 0
    assert lib.mst_roll_slices(2 ** 31 - 1) == 2 ** 21
    count = lambda x_, n, nfeat, mode, ws_: lib.mst_roll_count(x_, n, nfeat, mode, ws_, None)
    for args in ((None, 10, 5, 0, P(ws)), (P(x), 10, 5, 0, None), (P(x), 0, 5, 0, P(ws)), (P(x), 2 ** 31, 5, 0, P(ws)),
                 (P(x), 10, 3, 0, P(ws)), (P(x), 10, 0, 0, P(ws)), (P(x), 10, 5, 2, P(ws)), (P(x), 10, 5, -1, P(ws)),
                 (P(x) + 2, 9, 5, 0, P(ws))):
        assert count(*args) == -1, args                          # MST_ERR_ARG
    assert ws.tolist() == [-7, -7]
    assert count(P(x), 10, 5, 0, P(ws)) == 0 and ws.tolist() == [0, 10]
    compact = lambda x_, n, nfeat, mode, ws_, cap, c, f: lib.mst_roll_compact(x_, n, nfeat, mode, ws_, cap, c, f, None)
    ok = (P(x), 10, 5, 0, P(ws), 10, P(cells), P(feats))
    for at, bad in ((0, None), (4, None), (6, None), (7, None), (1, 0), (1, 2 ** 31), (2, 3), (2, 4), (3, 2), (3, -1), (5, -1),
                    (0, P(x) + 1)):
        args = ok[:at] + (bad,) + ok[at + 1:]
        assert compact(*args) == -1, args
    assert (cells == -7).all() and torch.isnan(feats).all()      # outputs untouched
    assert compact(*ok) == 0 and cells.tolist() == list(range(10)) and _same_bits(feats.view(10, 5), x)


# ---- 10
def _predictions(seed, C, R, T):
    """Rolls like a model's predictions: soft accidentals, a third of the live velocities around the .01 threshold."""
    clip = synth_clip(seed, C, R, T, True, density=.03)
    g = torch.Generator().manual_seed(seed)
    pitched, unpitched = clip['pitched'].clone(), clip['unpitched'].clone()
    for x in (pitched, unpitched):
        quiet = torch.rand(x.shape[:-1], generator=g) < .3
        x[..., 1] = torch.where(quiet, x[..., 1] * .02, x[..., 1])
    live = (pitched[..., 1:2] != 0).float()
    pitched[..., 2:] = torch.rand(pitched.shape[:-1] + (3,), generator=g) * live
    return pitched, unpitched


def test_host_decode_from_records(tmp_path):
    from oracle import style_oracle as so
    from style.midi import create_midi
    from style.midi_conversion import ChannelConverter
    from style.style_transfer import channel_slots, decode_records, decode_rolls, get_model_input
    _, (info, _, _, instruments, _) = get_model_input(os.path.join(HERE, 'golden', 'midi', 'Dancing in the Moonlight.mid'))
    C, R, T = 3, 5, 4
    assert len(instruments) >= C
    cc = ChannelConverter(info)
    infos, uinfo = channel_slots(instruments[:C])
    pitched, unpitched = _predictions(17, C, R, T)
    hard_p, hard_u = so.hard_output(pitched.clone()).numpy()[0], so.hard_output(unpitched.clone()).numpy()[0, 0]
    assert 0 < (hard_p[..., 1] != 0).sum() < (pitched[..., 1] != 0).sum()           # the threshold does drop notes
    rec_p, rec_u = _compact(pitched, 'hard'), _compact(unpitched, 'hard')
    per = R * T * 10 * 56
    cuts = np.searchsorted(rec_p.cells.numpy(), per * np.arange(C + 1))
    pairs = [(cc.records2qchannel(infos[c], (R, T, 10, 56), rec_p.cells.numpy()[cuts[c]:cuts[c + 1]] - c * per,
                                  rec_p.feats.numpy()[cuts[c]:cuts[c + 1]]), cc.vchannel2qchannel(infos[c], hard_p[c]))
             for c in range(C)]
    pairs.append((cc.records2qchannel(uinfo, (R, T, 10, 47, 2), rec_u.cells.numpy(), rec_u.feats.numpy()),
                  cc.vchannel2qchannel(uinfo, hard_u)))
    for got, want in pairs:
        assert {k: v for k, v in got.items() if k != 'notes'} == {k: v for k, v in want.items() if k != 'notes'}
        a, b = got['notes'].__dict__, want['notes'].__dict__
        assert len(want['notes']) > 20 and set(a) == set(b)
        for name in b:                                           # every column, value and dtype
            assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, name
            assert np.ascontiguousarray(a[name]).tobytes() == np.ascontiguousarray(b[name]).tobytes(), name
    files = [str(tmp_path / 'records.mid'), str(tmp_path / 'rolls.mid')]
    create_midi(info, *[cc.qchannel2channel(ci, q) for ci, (q, _) in zip(infos + [uinfo], pairs)], max_delta_time=1).save(files[0])
    decode_rolls(cc, infos, hard_p, uinfo, hard_u).save(files[1])
    third = str(tmp_path / 'driver.mid')
    decode_records(cc, infos, rec_p, uinfo, rec_u).save(third)
    data = [open(f, 'rb').read() for f in files + [third]]
    assert len(data[1]) > 1000 and data[0] == data[1] and data[2] == data[1]
    # fewer channel infos than channels (save's shape[1] quirk): the same channels are kept
    decode_records(cc, infos[:2], rec_p, uinfo, rec_u).save(files[0])
    decode_rolls(cc, infos[:2], hard_p, uinfo, hard_u).save(files[1])
    assert open(files[0], 'rb').read() == open(files[1], 'rb').read() != data[1]


# ---- 11
def test_from_packed_adopts_and_validates():
    from style.data import SparseRoll, sparsify
    x = synth_clip(5, 2, 2, 2, True, density=.1)['unpitched']
    roll = sparsify(x, pin=False)
    packed = roll.packed.clone()
    again = SparseRoll.from_packed(packed, x.shape)
    assert again.packed.data_ptr() == packed.data_ptr() and again.cells.data_ptr() == packed.data_ptr() + 16     # no copy
    assert again.count == roll.count and again.shape == roll.shape and again.nfeat == 2 and again.n_cells == roll.n_cells
    assert torch.equal(again.cells, roll.cells) and _same_bits(again.feats, roll.feats)
    assert np.array_equal(again.to_numpy().view(np.uint32), x.numpy().view(np.uint32))
    bad = packed.clone()
    bad[4], bad[5] = int(packed[5]), int(packed[4])              # descending cells
    with pytest.raises(ValueError):
        SparseRoll.from_packed(bad, x.shape)
    bad = packed.clone()
    bad[4 + roll.count - 1] = roll.n_cells                       # out of range
    with pytest.raises(ValueError):
        SparseRoll.from_packed(bad, x.shape)
    with pytest.raises(ValueError):
        SparseRoll.from_packed(packed[:-1].clone(), x.shape)     # not the size its count asks for
    with pytest.raises(ValueError):
        SparseRoll.from_packed(packed, x.shape[:-1] + (3,))      # neither pitched nor unpitched
    with pytest.raises(ValueError):
        SparseRoll.from_packed(packed.float(), x.shape)


# ---- 12
@pytest.mark.parametrize('mode', [NONZERO, HARD])
def test_two_runs_give_identical_bytes(mode):
    x = synth_clip(12, 2, 3, 2, True, density=.3)['pitched']
    first, second = _raw(x, mode), _raw(x, mode)
    assert int(first[0][-1]) > 1000
    for a, b in zip(first, second):
        assert torch.equal(_bits(a), _bits(b))


def test_compact_rejects_a_bad_mode_and_shape():
    from style.data import compact
    with pytest.raises(ValueError):
        compact(torch.zeros(4, 10, 5), 'soft', native=_native())
    with pytest.raises(ValueError):
        compact(torch.zeros(4, 10, 3), 'hard', native=_native())


def test_hard_output_sparse_has_no_cpu_fallback():
    from style import _native
    from style.model import hard_output_sparse
    with pytest.raises(_native.MstError, match='GPU tensor'):
        hard_output_sparse(torch.zeros(1, 1, 1, 1, 10, 56, 5))
