"""Windowed evaluation on the CPU: mst_window_inputs and mst_eval_accumulate (the product's kernel source on the hipsim
interpreter, the cases of tests/eval_window_cases.py), their composition with mst_clip_window and mst_eval_iteration, and the host
side — SongStore's fixed set of windows, its padded batches, and round_result."""
import numpy as np
import pytest
import torch

import eval_window_cases as wc
import simutil


@pytest.mark.parametrize('case', wc.KERNEL_CASES, ids=[c.__name__[5:] for c in wc.KERNEL_CASES])
def test_kernels(case):
    case(simutil.sim_native(), 'cpu')


def test_composition_at_the_c_abi():
    wc.case_composition(simutil.sim_native(), 'cpu', K=3)


# ---- SongStore, host only
def _sounding(clip, r0, bars):
    """The silence rule on the dense rolls: a sounding pitched note and a sounding unpitched one in bars [r0, r0 + bars)."""
    return bool(np.any(clip['pitched'][:, :, r0:r0 + bars].numpy()) and np.any(clip['unpitched'][:, :, r0:r0 + bars].numpy()))


def _expected(clips, bars, stride):
    """(windows, skipped) from the dense rolls with numpy, not from window_sounds."""
    found, skipped = [], 0
    for s, clip in enumerate(clips):
        R = clip['pitched'].shape[2]
        for r0 in range(0, R - bars + 1, stride):
            if _sounding(clip, r0, bars):
                found.append((s, r0))
            else:
                skipped += 1
    return found, skipped


def test_windows_enumerate_every_song():
    store = wc.make_store('cpu')
    found = store.windows(2)
    assert list(found) == [(0, 0), (1, 0), (1, 2), (2, 0), (3, 0), (3, 2), (4, 0)] and found.skipped == 0
    assert (list(found), found.skipped) == _expected(wc.songs(), 2, 2)
    every = store.windows(2, stride=1)
    assert len(every) == 12 and (list(every), every.skipped) == _expected(wc.songs(), 2, 1)
    assert list(store.windows(2)) == list(found) and list(store.windows(2, stride=1)) == list(every)      # deterministic
    assert list(store.windows(5)) == [(1, 0)] and list(store.windows(6)) == []
    with pytest.raises(ValueError):
        store.windows(0)
    with pytest.raises(ValueError):
        store.windows(2, stride=0)


def test_window_batches_pad_the_last_batch():
    store = wc.make_store('cpu')
    batches = store.window_batches(2, 3)
    assert [live for _, live in batches] == [3, 3, 1] and batches.skipped == 0
    assert all(b.K == 3 and (b.C, b.bars, b.T, b.percussion) == (2, 2, 2, True) for b, _ in batches)
    flat = [(s, r) for b, _ in batches for s, r in zip(b.songs.tolist(), b.r0s.tolist())]
    assert flat == [(0, 0), (1, 0), (1, 2), (2, 0), (3, 0), (3, 2), (4, 0), (4, 0), (4, 0)]           # padded with its last window
    again = store.window_batches(2, 3)
    assert [(b.songs.tolist(), b.r0s.tolist(), live) for b, live in again] == [(b.songs.tolist(), b.r0s.tolist(), live) for b, live in batches]
    assert [live for _, live in store.window_batches(2, 7)] == [7] and [live for _, live in store.window_batches(2, 8)] == [7]
    assert [live for _, live in store.window_batches(2, 4, stride=1)] == [4, 4, 4]
    with pytest.raises(ValueError):
        store.window_batches(2, 0)


def test_batches_are_cut_per_bucket():
    """Songs of two shapes: each bucket's windows fill batches of their own, buckets in sorted key order, songs ascending."""
    from tools.synth import synth_clip
    clips = list(wc.songs()[:2])
    solo = synth_clip(77, 1, 4, 2, True, density=.05)
    store = wc.make_store('cpu', [clips[0], solo, clips[1]])
    assert list(store.windows(2)) == [(1, 0), (1, 2), (0, 0), (2, 0), (2, 2)]              # bucket (1, 2, True) sorts first
    got = [((b.C, b.T, b.percussion), b.songs.tolist(), b.r0s.tolist(), live) for b, live in store.window_batches(2, 2)]
    assert got == [((1, 2, True), [1, 1], [0, 2], 2), ((2, 2, True), [0, 2], [0, 0], 2), ((2, 2, True), [2, 2], [2, 2], 1)]


def test_a_silent_window_is_left_out_and_counted():
    """Song 1 (5 bars) with bars 2-3 zeroed loses exactly the window at bar 2 (stride 2), and the windows at bars 1, 2, 3 keep
    or lose theirs as the dense rolls say (stride 1)."""
    clips = [dict(c) for c in wc.songs()]
    for key in ('pitched', 'unpitched'):
        x = clips[1][key].clone()
        x[:, :, 2:4] = 0.
        clips[1][key] = x
    store = wc.make_store('cpu', clips)
    found = store.windows(2)
    assert list(found) == [(0, 0), (1, 0), (2, 0), (3, 0), (3, 2), (4, 0)] and found.skipped == 1
    assert (list(found), found.skipped) == _expected(clips, 2, 2)
    every = store.windows(2, stride=1)
    assert (list(every), every.skipped) == _expected(clips, 2, 1) and every.skipped == 1 and (1, 2) not in every
    batches = store.window_batches(2, 4)
    assert [live for _, live in batches] == [4, 2] and batches.skipped == 1
    # percussion alone silent in a stretch: the window goes as well (the loss's masked means would be 0 / 0)
    clips[3]['unpitched'] = clips[3]['unpitched'].clone()
    clips[3]['unpitched'][:, :, 0:2] = 0.
    found = wc.make_store('cpu', clips).windows(2)
    assert (3, 0) not in found and (3, 2) in found and found.skipped == 2 and (list(found), 2) == _expected(clips, 2, 2)


# ---- round_result, host only
def test_round_result():
    from style import _native as nat
    from style.metrics import nanmean_leaves, round_result, validation_row, NoteMetrics, SongInfoMetrics
    losses, metrics = wc.batch_values(5, 2, seed=5, no_percussion=(1, 4))
    metrics[:, :, 7] = 0.
    metrics = np.floor(metrics)
    acc = wc.fold(np.zeros(41), losses, metrics, None)
    res = round_result(torch.from_numpy(acc))
    assert res['clips'] == 5 and res['losses'].shape == (15,)
    want = np.array([acc[2 + i] / (acc[1] if 7 <= i < 11 else acc[0]) for i in range(15)])
    assert acc[0] == 5 and acc[1] == 3 and wc.same_doubles(res['losses'], want)
    # nanmean_leaves' rule: which clips enter which mean.  (Its sums associate differently, so its last bits may differ: the
    # two are compared on leaves made of small integers, where every sum is exact.)
    whole = np.floor(losses * 8)
    whole[[1, 4], 7:11] = np.nan
    assert wc.same_doubles(round_result(wc.fold(np.zeros(41), whole.astype(np.float32), metrics, None))['losses'], nanmean_leaves(whole))
    m = torch.from_numpy(metrics)
    assert torch.equal(res['pitched'].words, NoteMetrics(m[:, :2]).sum().words)
    assert torch.equal(res['unpitched'].words, NoteMetrics(m[:, 2]).sum().words)
    assert torch.equal(res['song_info'].words, SongInfoMetrics.from_device(m[:, 3]).sum().words) and res['song_info'].words[7] == 5
    row = validation_row(3, res['clips'], res['losses'], res['pitched'], res['unpitched'], res['song_info'])
    assert row['clips'] == 5 and row['iteration'] == 3 and row['total'] == res['losses'][0]
    # nobody has percussion: the unpitched leaves are NaN, the others are not; an empty round is all NaN
    losses, metrics = wc.batch_values(3, 2, seed=6, no_percussion=(0, 1, 2))
    res = round_result(wc.fold(np.zeros(41), losses, metrics, None))
    assert np.isnan(res['losses'][7:11]).all() and np.isfinite(np.delete(res['losses'], range(7, 11))).all()
    res = round_result(np.zeros(41))
    assert res['clips'] == 0 and np.isnan(res['losses']).all()
    with pytest.raises(ValueError):
        round_result(np.zeros(40))
    assert nat.EVAL_ACC_WORDS == 41


def test_cli_option():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('train_model_cli', os.path.join(simutil.ROOT, 'train-model.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.split_options(['--batch-clips', '8', '--eval-windows', '5', 'data', '3']) == (['data', '3'], dict(batch_clips=8, eval_windows=5))
    with pytest.raises(SystemExit):
        cli.split_options(['--eval-windows', '5'])
