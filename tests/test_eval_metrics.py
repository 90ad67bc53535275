"""Held-out evaluation on the CPU: mst_roll_metrics and mst_eval_iteration (the product's kernel source on the hipsim
interpreter) against the numpy yardstick of tests/eval_cases.py, and the host-only pieces — NoteMetrics arithmetic, the
validation CSV, the held-out file split — which need no library at all."""
import csv
import math

import numpy as np
import pytest
import torch

import eval_cases as ec
import parity_cases as pc
import simutil


def _native():
    native = simutil.sim_native()
    assert native.roll_slices(ec.S) == 1 and native.roll_slices(ec.S + 1) == 2, 'eval_cases.S is not the kernels\' slice'
    return native


# ---- mst_roll_metrics
@pytest.mark.parametrize('nfeat', [5, 2])
@pytest.mark.parametrize('n_groups,group_cells', ec.SIZES)
def test_sizes(n_groups, group_cells, nfeat):
    ec.size_case(_native(), 'cpu', n_groups, group_cells, nfeat)


@pytest.mark.parametrize('nfeat', [5, 2])
def test_more_partials_than_the_finishing_workgroup_has_lanes(nfeat):
    ec.size_case(_native(), 'cpu', *ec.MANY_PARTIALS, nfeat)


@pytest.mark.parametrize('nfeat', [5, 2])
def test_pred_and_target_at_different_misalignments(nfeat):
    ec.misaligned_case(_native(), 'cpu', nfeat)


@pytest.mark.parametrize('nfeat', [5, 2])
def test_two_runs_give_identical_bits(nfeat):
    ec.two_runs_case(_native(), 'cpu', nfeat)


@pytest.mark.parametrize('nfeat', [5, 2])
def test_edge_values(nfeat):
    ec.edge_case(_native(), 'cpu', nfeat)


@pytest.mark.parametrize('key', ['pitched', 'unpitched'])
def test_synthetic_rolls_around_the_threshold(key):
    ec.synth_case(_native(), 'cpu', key)


def test_err_arg_cases():
    ec.err_arg_case(_native(), 'cpu')


# ---- mst_eval_iteration
@pytest.mark.parametrize('unp', [True, False])
def test_eval_iteration_small(unp):
    ec.eval_case(_native(), 'cpu', pc.SMALL, 3, 2, 3, unp)


@pytest.mark.parametrize('gemm_tile', [None, 64])
def test_eval_iteration_three_clips(gemm_tile):
    ec.eval_case(_native(), 'cpu', pc.SMALL, 2, 2, 1, True, K=3, gemm_tile=gemm_tile)


def test_eval_iteration_full_widths():
    ec.eval_case(_native(), 'cpu', pc.FULL, 2, 2, 2, True)


def test_eval_iteration_refusals():
    ec.eval_refusals(_native(), 'cpu')


# ---- host only
def _record(*words):
    return torch.tensor(words, dtype=torch.float64)


def test_note_metrics_arithmetic():
    from style.metrics import NoteMetrics
    m = NoteMetrics(_record(100, 8, 10, 6, 3, 1.5, 3., 0))
    assert (m.precision, m.recall, m.accidentals_accuracy, m.velocity_mae, m.duration_mae) == (.75, .6, .5, .25, .5)
    assert m.f1 == 12 / 18 and abs(m.f1 - 2 * .75 * .6 / (.75 + .6)) < 1e-15
    empty = NoteMetrics.zeros()
    for k in NoteMetrics.fields:
        assert math.isnan(getattr(empty, k)), k                 # 0 / 0 is NaN, not a score
    silent = NoteMetrics(_record(100, 0, 10, 0, 0, 0, 0, 0))   # nothing predicted: recall 0, precision undefined
    assert math.isnan(silent.precision) and silent.recall == 0. and silent.f1 == 0. and math.isnan(silent.velocity_mae)
    with pytest.raises(ValueError):
        NoteMetrics(torch.zeros(7, dtype=torch.float64))
    with pytest.raises(ValueError):
        NoteMetrics(torch.zeros(8))                             # float32 cannot hold the counts of a long song exactly


def test_records_add_to_micro_averages():
    from style.metrics import NoteMetrics, SongInfoMetrics
    a, b = NoteMetrics(_record(100, 8, 10, 6, 3, 1.5, 3., 0)), NoteMetrics(_record(50, 2, 10, 2, 2, .5, 0., 0))
    s = a + b
    assert s.words.tolist() == [150, 10, 20, 8, 5, 2., 3., 0] and s.precision == .8 and s.recall == .4
    assert sum([a, b]).words.tolist() == s.words.tolist()
    per_channel = NoteMetrics(torch.stack([a.words, b.words, NoteMetrics.zeros().words]))
    assert per_channel.sum().words.tolist() == s.words.tolist()
    prec = per_channel.precision
    assert prec.shape == (3,) and prec[:2].tolist() == [.75, 1.] and math.isnan(float(prec[2]))
    with pytest.raises(TypeError):
        a + SongInfoMetrics.zeros()
    x = SongInfoMetrics.from_device(_record(41, 5, 4, 3, 1, 12., 0, 0))
    y = SongInfoMetrics.from_device(_record(41, 1, 2, 1, 0, 4., 0, 0))
    t = x + y
    assert (t.instruments_precision, t.instruments_recall, t.mode_accuracy, t.bpm_mae) == (4 / 6, 4 / 6, .5, 8.)
    assert t.instruments_f1 == 8 / 12
    assert math.isnan(SongInfoMetrics.zeros().mode_accuracy)


def test_validation_csv(tmp_path):
    from style import _native
    from style.metrics import (NoteMetrics, SongInfoMetrics, VALIDATION_FIELDS, append_validation_rows, nanmean_leaves,
                               validation_row)
    leaves = np.arange(15, dtype=np.float64)[None].repeat(2, 0)
    leaves[1] += 2
    leaves[1, 7:11] = np.nan                                      # the second clip has no percussion
    mean = nanmean_leaves(leaves)
    assert mean[0] == 1. and mean[6] == 7. and mean[7] == 7. and mean[11] == 12.
    assert np.isnan(nanmean_leaves(leaves[1:])[7]) and nanmean_leaves(leaves[1:])[0] == 2.
    leaves[0, 0] = np.nan
    assert np.isnan(nanmean_leaves(leaves)[0])                    # a NaN loss is not averaged away
    pitched = NoteMetrics(_record(100, 8, 10, 6, 3, 1.5, 3., 0))
    song = SongInfoMetrics.from_device(_record(41, 5, 4, 3, 1, 12., 0, 0))
    path = str(tmp_path / 'log' / 'validation.csv')
    append_validation_rows(path, [validation_row(1, 2, mean, pitched, NoteMetrics.zeros(), song)])
    append_validation_rows(path, [validation_row(3, 2, nanmean_leaves(leaves[1:]), pitched, pitched, song)])
    rows = list(csv.DictReader(open(path)))
    assert len(rows) == 2 and list(rows[0].keys()) == VALIDATION_FIELDS            # one header
    assert VALIDATION_FIELDS[:2] == ['iteration', 'clips'] and VALIDATION_FIELDS[2:17] == _native.LOSS_KEYS
    assert len(VALIDATION_FIELDS) == 17 + 6 + 5 + 5 and 'unpitched_accidentals_accuracy' not in VALIDATION_FIELDS
    assert rows[0]['iteration'] == '1' and rows[0]['clips'] == '2' and rows[0]['total'] == '1.0'
    assert rows[0]['pitched_precision'] == '0.75' and rows[0]['unpitched_f1'] == 'nan' and rows[0]['mode_accuracy'] == '1.0'
    assert rows[1]['channels_loss_unpitched_total'] == '' and rows[1]['unpitched_recall'] == '0.6' and rows[1]['bpm_mae'] == '12.0'


def test_held_out_files_are_the_last_of_the_sorted_list():
    from style.train import split_eval_files
    files = ['c.mid', 'a.mid', 'd.mid', 'b.mid']
    assert split_eval_files(files, 1) == (['a.mid', 'b.mid', 'c.mid'], ['d.mid'])
    assert split_eval_files(files, 0) == (sorted(files), [])
    assert split_eval_files(files, 9) == ([], sorted(files))


def test_note_metrics_has_no_cpu_fallback():
    from style import _native
    from style.metrics import note_metrics
    with pytest.raises(_native.MstError, match='GPU tensors'):
        note_metrics(torch.zeros(1, 1, 1, 1, 10, 56, 5), torch.zeros(1, 1, 1, 1, 10, 56, 5))
