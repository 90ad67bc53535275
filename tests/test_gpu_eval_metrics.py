"""-m gpu: the held-out evaluation path on an MI355X.  The cases of tests/eval_cases.py (mst_roll_metrics and
mst_eval_iteration against the numpy yardstick, bit-equal losses / predictions / repeat runs), the two launches replayed from
a captured graph, and the Python surface: StyleTransferModel.eval_iteration, style.metrics.note_metrics and the evaluation
rounds of style.train.train, which must leave the training bits alone."""
import csv
import os

import numpy as np
import pytest
import torch

import eval_cases as ec
import parity_cases as pc
from tools.synth import synth_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


def _native():
    from style import _native
    native = _native.get()
    assert native.roll_slices(ec.S) == 1 and native.roll_slices(ec.S + 1) == 2, 'eval_cases.S is not the kernels\' slice'
    return native


# ---- mst_roll_metrics
@pytest.mark.parametrize('nfeat', [5, 2])
@pytest.mark.parametrize('n_groups,group_cells', ec.SIZES + [ec.MANY_PARTIALS])
def test_sizes(n_groups, group_cells, nfeat):
    ec.size_case(_native(), DEV, n_groups, group_cells, nfeat)


@pytest.mark.parametrize('nfeat', [5, 2])
def test_pred_and_target_at_different_misalignments(nfeat):
    ec.misaligned_case(_native(), DEV, nfeat)


@pytest.mark.parametrize('nfeat', [5, 2])
def test_two_runs_give_identical_bits(nfeat):
    ec.two_runs_case(_native(), DEV, nfeat)


@pytest.mark.parametrize('nfeat', [5, 2])
def test_edge_values(nfeat):
    ec.edge_case(_native(), DEV, nfeat)


@pytest.mark.parametrize('key', ['pitched', 'unpitched'])
def test_synthetic_rolls_around_the_threshold(key):
    ec.synth_case(_native(), DEV, key)


def test_err_arg_cases():
    ec.err_arg_case(_native(), DEV)


def test_bench_shape_pitched_roll_as_four_channel_groups():
    pred, target, n_groups, group_cells = ec.synth_pair('pitched', seed=1, crt=(4, 16, 4))
    assert (n_groups, group_cells) == (4, 35840) and group_cells % ec.S == 0          # whole slices
    got = ec.metrics_case(_native(), DEV, pred, target, n_groups, group_cells, 5, leads=((0, 0), (1, 3)))
    assert all(ec.counts_not_trivial(got[g].numpy()) for g in range(4))


def test_more_groups_than_one_launch_takes():
    # 65535 groups go into one launch's blockIdx.y; the rest follow in a second launch of the same chain
    n_groups, group_cells = 65535 + 2, 3
    pred, target = ec.random_pair(n_groups * group_cells, 2, seed=5)
    ec.metrics_case(_native(), DEV, pred, target, n_groups, group_cells, 2)


def test_the_two_launches_replay_from_a_captured_graph():
    from style import _native as nat
    native = _native()
    pairs = [ec.synth_pair('pitched', seed=s, crt=(4, 16, 4)) for s in (1, 2)]
    n_groups, group_cells = pairs[0][2:]
    pred, target = pairs[0][0].to(DEV), pairs[0][1].to(DEV)
    scratch = torch.full((native.roll_metrics_scratch_bytes(n_groups, group_cells) // 8,), NAN, dtype=torch.float64, device=DEV)
    out = torch.full((n_groups, ec.W), NAN, dtype=torch.float64, device=DEV)
    native.roll_metrics(pred, target, n_groups, group_cells, 5, scratch, out, nat.current_stream(DEV))      # (loads the code objects)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # a single chain on the capture stream
        native.roll_metrics(pred, target, n_groups, group_cells, 5, scratch, out, nat.current_stream(DEV))
    seen = []
    for p, t, _, _ in pairs:
        pred.copy_(p)
        target.copy_(t)
        out.fill_(NAN)
        scratch.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        eager = ec.run_metrics(native, DEV, p, t, n_groups, group_cells, 5)
        assert ec.same_bits(out, eager) and ec.counts_not_trivial(eager.numpy())
        seen.append(out.cpu().clone())
    assert not ec.same_bits(seen[0], seen[1])


# ---- mst_eval_iteration
@pytest.mark.parametrize('unp', [True, False])
def test_eval_iteration_small(unp):
    ec.eval_case(_native(), DEV, pc.SMALL, 3, 2, 3, unp)


@pytest.mark.parametrize('gemm_tile', [None, 64])
def test_eval_iteration_three_clips(gemm_tile):
    ec.eval_case(_native(), DEV, pc.SMALL, 2, 2, 1, True, K=3, gemm_tile=gemm_tile)


def test_eval_iteration_full_widths():
    ec.eval_case(_native(), DEV, pc.FULL, 2, 2, 2, True)


def test_eval_iteration_bench_shape_on_the_twelve_workgroup_lstm():
    from style import _native as nat
    from test_lstm_multi import lstm_steps
    native = _native()
    plan = nat.Plan(native, pc.make_dims(pc.FULL, 4, 16, 4, True), DEV)
    assert [s[3] for s in lstm_steps(plan)] == [1]              # the default flavours take the multi-workgroup kernels here
    del plan
    ec.eval_case(native, DEV, pc.FULL, 4, 16, 4, True)


def test_eval_iteration_refusals():
    ec.eval_refusals(_native(), DEV)


# ---- the Python surface
def _clip_args(clip):
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in clip.items()}
    return (d['mode'], d['bpm'], d['pitched'], d['instruments_features'], d['unpitched'], d['used_instruments'], d['bpm_int'])


def _spread_velocities(model):
    """A freshly built model predicts every cell "on"; as in eval_cases.eval_params the appliers' last Linear is scaled by 20 and
    its velocity bias moved by -4.6.  Checked with the oracle on the CPU: the seed-108 FULL model then gives 68 / 54 true
    positives of 1084 / 1120 predicted and 124 / 100 target notes in the two channels of clip 5, and 43 of 960 and 88 unpitched."""
    with torch.no_grad():
        for applier in (model.pitched_style_applier, model.unpitched_style_applier):
            applier.linear.weight *= 20.
            applier.linear.bias[1] += -4.6


def test_model_eval_iteration():
    from style.data import sparsify
    from style.metrics import note_metrics
    from test_host_surface import FULL, build_model
    model = build_model(FULL, seed=108).to(DEV)
    _spread_velocities(model)
    clip = synth_clip(5, 2, 2, 2, True, density=.05)
    args = _clip_args(clip)
    res = model.eval_iteration(*args)
    assert res.losses.device.type == 'cuda' and res.metrics.device.type == 'cuda' and tuple(res.metrics.shape) == (4, 8)
    assert res.metrics.dtype == torch.float64
    row = model.train_iteration(*args)
    assert ec.same_bits(res.losses, row)                         # the same loss row as train_iteration
    with torch.no_grad():
        _, xp, xu = model(*args[:5])
    per_channel = note_metrics(xp, args[2], per_channel=True)
    assert ec.same_bits(per_channel.words, res.metrics[:2]) and ec.same_bits(note_metrics(xu, args[4]).words, res.metrics[2])
    assert ec.same_bits(note_metrics(xp, args[2]).words, res.metrics[:2].sum(0))
    for m in (res.pitched.sum().cpu(), res.unpitched.cpu()):
        assert ec.counts_not_trivial(m.words.numpy()) and 0 < m.precision < 1 and 0 < m.recall < 1 and 0 < m.f1 < 1
    assert res.song_info.cpu().words[0] == 41 and res.song_info.cpu().words[7] == 1
    # a SparseRoll input gives the same bits as the dense one
    sparse = model.eval_iteration(args[0], args[1], sparsify(clip['pitched']), args[3], sparsify(clip['unpitched']), args[5], args[6])
    assert ec.same_bits(sparse.losses, res.losses) and ec.same_bits(sparse.metrics, res.metrics)
    # pitched only: the unpitched record is all zero
    solo = synth_clip(6, 2, 2, 2, False, density=.05)
    res = model.eval_iteration(*_clip_args(solo))
    assert not res.metrics[2].cpu().any() and torch.isnan(res.losses[7:11]).all() and torch.isfinite(res.losses[0])


def test_evaluation_between_two_accumulation_iterations_changes_nothing():
    from style.optim import FusedAdam
    from test_host_surface import FULL, build_model
    clips = [_clip_args(synth_clip(5 + k, 2, 2, 2, True, density=.05)) for k in range(3)]
    left = {}
    for with_eval in (True, False):
        model = build_model(FULL, seed=108).to(DEV)
        opt = FusedAdam(model, lr=.01, step_size=200, gamma=.9)
        opt.zero_grad()
        rows = []
        for step in range(2):                                    # the second step replays the lanes' captured graphs
            rows.append(model.train_iteration(*clips[0]))          # a row of its lane's ring: read after the lanes are joined
            if with_eval:
                res = model.eval_iteration(*clips[2])
                assert torch.isfinite(res.losses[0])
            rows.append(model.train_iteration(*clips[1]))
            opt.step()
        torch.cuda.synchronize()
        left[with_eval] = [t.clone() for t in [model._flat, opt.exp_avg, opt.exp_avg_sq, opt.state] + rows]
    assert float(left[True][3][0]) == 2 and all(torch.isfinite(row[0]) and row[0] > 0 for row in left[True][4:])
    for a, b in zip(left[True], left[False]):
        assert ec.same_bits(a, b)


def test_train_with_evaluation_rounds(tmp_path):
    from style import style_transfer as st
    from style.metrics import VALIDATION_FIELDS
    from style.train import build_model, train
    from test_train_driver import SONGS
    songs = [st.get_model_input(p) for p in SONGS]
    out = {}
    for with_eval in (True, False):
        d = tmp_path / str(int(with_eval))
        model = build_model(seed=108)
        kwargs = dict(eval_inputs=iter(songs[::-1] * 2), eval_every=2, eval_clips=2, eval_info_path=str(d / 'validation.csv')) if with_eval else {}
        train(model, iter(songs + songs[:2]), n_iterations=6, iter_size=2, training_info_path=str(d / 'training.csv'), save_path=None,
              flush_every=4, progress=False, **kwargs)
        torch.cuda.synchronize()
        out[with_eval] = (open(d / 'training.csv', 'rb').read(), model._flat.clone())
    assert len(out[True][0]) > 500 and out[True][0] == out[False][0] and ec.same_bits(out[True][1], out[False][1])
    assert not os.path.exists(tmp_path / '0' / 'validation.csv')
    rows = list(csv.DictReader(open(tmp_path / '1' / 'validation.csv')))
    assert len(rows) == 3 and list(rows[0].keys()) == VALIDATION_FIELDS
    assert [r['iteration'] for r in rows] == ['1', '3', '5'] and all(r['clips'] == '2' for r in rows)
    for r in rows:
        for k in ('pitched_precision', 'pitched_recall', 'pitched_f1'):
            assert np.isfinite(float(r[k])) and 0. <= float(r[k]) <= 1., (k, r[k])
        assert np.isfinite(float(r['total'])) and float(r['total']) > 0
