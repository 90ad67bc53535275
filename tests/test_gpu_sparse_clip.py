"""-m gpu: the sparse input path on an MI355X.  A clip fed as note records (style.data.SparseRoll, expanded on the device by
mst_clip_scatter) must give the very bits a dense clip gives: the scatter itself, the fused training loop on both
accumulation lanes (eager, capture and replay), the autograd surface, and style.train.train's CSV."""
import csv

import numpy as np
import pytest
import torch

from tools.synth import synth_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sparse(clip):
    from style.data import sparsify
    return sparsify(clip['pitched']), (None if clip['unpitched'] is None else sparsify(clip['unpitched']))


@pytest.mark.parametrize('crt', [(4, 16, 4), (8, 151, 4)])
def test_scatter_is_bit_equal(crt):
    clip = synth_clip(1, *crt, True)
    for x, roll in zip((clip['pitched'], clip['unpitched']), _sparse(clip)):
        out = torch.full(x.shape, float('nan'), device=DEV)
        got = roll.to_dense(DEV, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(_bits(got.cpu()), _bits(x))
        fresh = roll.to_dense(DEV)
        assert fresh.shape == x.shape and torch.equal(_bits(fresh.cpu()), _bits(x))


def test_train_iteration_fed_sparse_equals_fed_dense():
    from style.optim import FusedAdam
    from style.train import build_model
    clips = [synth_clip(k, 2, 3, 2, True) for k in (11, 12)]
    rows = {}
    for feed in ('dense', 'sparse'):
        model = build_model(seed=108)
        opt = FusedAdam(model)                             # switches the two accumulation lanes on
        opt.zero_grad()
        got = []
        for it in range(8):                                # per lane: eager, capture + replay, replay, replay; the clips alternate per lane
            clip = clips[(it // 2) % 2]
            small = [clip[k].to(DEV) for k in ('mode', 'bpm', 'instruments_features', 'used_instruments')]
            if feed == 'sparse':
                pitched, unpitched = _sparse(clip)
            else:
                pitched, unpitched = clip['pitched'].to(DEV), clip['unpitched'].to(DEV)
            got.append(model.train_iteration(small[0], small[1], pitched, small[2], unpitched, small[3], clip['bpm_int']))
        opt.step()                                         # joins the lanes: the loss rows (a ring per lane) may be read after it
        torch.cuda.synchronize()
        model.check_device_status()
        for lane in (0, 1):
            buffers = model.static_inputs(2, 3, 2, True, lane=lane)
            assert torch.equal(_bits(buffers[0].cpu()), _bits(clips[1]['pitched']))       # the last clip, and nothing else
            assert torch.equal(_bits(buffers[1].cpu()), _bits(clips[1]['unpitched']))
        rows[feed] = (torch.stack(got).cpu(), model._flat.detach().cpu().clone())
    assert torch.isfinite(rows['dense'][0][:, 0]).all()
    assert not torch.equal(rows['dense'][0][0], rows['dense'][0][2])                       # the two clips do differ
    assert torch.equal(_bits(rows['sparse'][0]), _bits(rows['dense'][0]))
    assert torch.equal(_bits(rows['sparse'][1]), _bits(rows['dense'][1]))


def test_unpinned_records_are_staged():
    """Records in pageable memory go through the lane's pinned staging slots (reused in turn, ordered by events)."""
    from style.data import SparseRoll
    from style.train import build_model
    clips = [synth_clip(k, 1, 2, 2, True) for k in (31, 32, 33)]
    model = build_model(seed=108)
    losses = {}
    for feed in ('dense', 'sparse'):
        model.zero_grad()
        got = []
        for it in range(6):
            clip = clips[it % 3]
            small = [clip[k].to(DEV) for k in ('mode', 'bpm', 'instruments_features', 'used_instruments')]
            notes = [clip['pitched'].to(DEV), clip['unpitched'].to(DEV)]
            if feed == 'sparse':
                notes = [SparseRoll(r.cells, r.feats, r.shape, pin=False) for r in _sparse(clip)]
                assert not notes[0].packed.is_pinned()
            got.append(model.train_iteration(small[0], small[1], notes[0], small[2], notes[1], small[3], clip['bpm_int']))
        torch.cuda.synchronize()
        losses[feed] = torch.stack(got).cpu()
    assert torch.equal(_bits(losses['sparse']), _bits(losses['dense']))


def test_forward_and_extract_style_take_sparse_rolls():
    from style.train import build_model
    model = build_model(seed=108)
    clip = synth_clip(21, 2, 2, 2, True)
    small = [clip[k].to(DEV) for k in ('mode', 'bpm', 'instruments_features')]
    dense = (clip['pitched'].to(DEV), clip['unpitched'].to(DEV))
    sparse = _sparse(clip)
    with torch.no_grad():
        for notes_a, notes_b in ((dense, sparse), ((dense[0], None), (sparse[0], None))):
            a = model.extract_style(small[0], small[1], notes_a[0], small[2], notes_a[1])
            b = model.extract_style(small[0], small[1], notes_b[0], small[2], notes_b[1])
            assert len(a) == 3 and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
            (ia, ma, ba), pa, ua = model(small[0], small[1], notes_a[0], small[2], notes_a[1])
            (ib, mb, bb), pb, ub = model(small[0], small[1], notes_b[0], small[2], notes_b[1])
            for x, y in ((ia, ib), (ma, mb), (ba, bb), (pa, pb)):
                assert torch.equal(_bits(x), _bits(y))
            assert (ua is None and ub is None) or torch.equal(_bits(ua), _bits(ub))
    # and through autograd: same gradients
    grads = []
    for notes in (dense, sparse):
        model.zero_grad()
        (_, _, _), xp, xu = model(small[0], small[1], notes[0], small[2], notes[1])
        (xp.sum() + xu.sum()).backward()
        grads.append(model._gflat.detach().cpu().clone())
    assert torch.equal(_bits(grads[0]), _bits(grads[1])) and float(grads[0].abs().sum()) > 0


def _songs():
    """Small synthetic songs in get_input's form: float64 rolls, one with silent percussion, one without pitched notes."""
    out = []
    for k, (C, R) in enumerate(((2, 3), (1, 4), (2, 3), (2, 3), (1, 4), (2, 3))):
        clip = synth_clip(40 + k, C, R, 4, True, density=.03)
        pitched, unpitched = clip['pitched'][0].double().numpy(), clip['unpitched'][0].double().numpy()
        if k == 1:
            unpitched[:] = 0.
        if k == 3:
            pitched[:] = 0.
        info = dict(bpm=90 + 7 * k, scale=dict(mode='major' if k % 2 else 'minor'))
        out.append((f'song{k}', (info, pitched, clip['instruments_features'][0].double().numpy(), list(range(C)), unpitched)))
    return out


@pytest.mark.parametrize('fused', [True, False])
def test_train_writes_the_same_csv_fed_sparse_or_dense(tmp_path, fused):
    from style.train import build_model, train
    rows = {}
    for sparse_input in (False, True):
        path = str(tmp_path / f'training_{int(sparse_input)}.csv')
        model = build_model(seed=108)
        train(model, iter(_songs()), n_iterations=6, iter_size=2, training_info_path=path, save_path=None, flush_every=4,
              progress=False, fused=fused, sparse_input=sparse_input)
        rows[sparse_input] = list(csv.reader(open(path)))
    assert len(rows[False]) == 1 + 5 and [r[0] for r in rows[False][1:]] == ['0', '1', '2', '4', '5']     # song 3 is skipped
    assert rows[False][2][8] == ''                                                                          # no percussion in song 1
    assert all(np.isfinite(float(r[1])) for r in rows[False][1:])
    assert rows[True] == rows[False]
