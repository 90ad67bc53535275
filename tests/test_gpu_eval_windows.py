"""-m gpu: windowed evaluation on an MI355X.  mst_window_inputs and mst_eval_accumulate (the cases of tests/eval_window_cases.py
on the gfx950 build) and their composition at the C ABI; StyleTransferModel.eval_windows against the batched plan fed
host-cropped dense clips (same plan, same input bits: same bits), eager and from its hipGraph; style.train.evaluate_windows
against the numpy fold of those; and that training is the same bits with or without evaluation rounds."""
import csv

import numpy as np
import pytest
import torch

import eval_cases as ec
import eval_window_cases as wc
import parity_cases as pc
from simutil import make_dims
from test_host_surface import build_model
from tools.synth import synth_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C, T, BARS = wc.C, wc.T, wc.BARS


def _native():
    from style import _native
    return _native.get()


@pytest.mark.parametrize('case', wc.KERNEL_CASES, ids=[c.__name__[5:] for c in wc.KERNEL_CASES])
def test_kernels(case):
    case(_native(), DEV)
    torch.cuda.synchronize()


def test_composition_at_the_c_abi():
    assert wc.case_composition(_native(), DEV, K=3) == 32
    torch.cuda.synchronize()


def test_the_two_launches_replay_from_a_captured_graph():
    """Rows and `live` are read on the device: one captured chain of the two launches serves other rows and a partial batch."""
    from style import _native as nat
    native = _native()
    tab = torch.from_numpy(wc.table().view(np.int32).copy()).to(DEV)
    fields = list(zip(wc.SRC, wc.LENS, wc.DST))
    K = 4
    rows = torch.zeros(K, dtype=torch.int32, device=DEV)
    ws = torch.full((wc.STRIDE * K,), wc.POISON, dtype=torch.int32, device=DEV)
    losses, metrics = wc.batch_values(K, 2, seed=51, no_percussion=(2,))
    dl, dm = torch.from_numpy(losses).to(DEV), torch.from_numpy(metrics).to(DEV)
    live = torch.zeros(1, dtype=torch.int32, device=DEV)
    acc = torch.zeros(wc.ACC, dtype=torch.float64, device=DEV)

    def body():
        native.window_inputs(tab, 6, wc.ROW_FLOATS, rows, K, fields, wc.STRIDE, ws, nat.current_stream(DEV))
        native.eval_accumulate(dl, dm, K, 2, live, acc, nat.current_stream(DEV))
    body()                                                       # (loads the code objects)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    want_acc = np.zeros(wc.ACC)
    for pick, n in (([5, 1, 1, 3], 4), ([0, 7, 2, 4], 1), ([2, 2, -1, 0], 3)):
        rows.copy_(torch.tensor(pick, dtype=torch.int32))
        live.fill_(n)
        ws.fill_(wc.POISON)
        before = ws.cpu().numpy().view(np.uint32).copy()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ws.cpu().numpy().view(np.uint32), wc.gather(before, 0, wc.table(), pick, fields, wc.STRIDE))
        want_acc = wc.fold(want_acc, losses, metrics, n)         # never zeroed in between: the replays accumulate
        assert wc.same_doubles(acc.cpu().numpy(), want_acc)
    assert want_acc[0] == 8


# ---- StyleTransferModel.eval_windows
def small_model():
    model = build_model(pc.SMALL, seed=7).to(DEV)
    with torch.no_grad():                                        # as eval_cases.eval_params: velocities spread over (0, 1)
        for applier in (model.pitched_style_applier, model.unpitched_style_applier):
            applier.linear.weight *= 20.
            applier.linear.bias[1] += -4.6
    model._sync_flat()
    return model


def batches(K):
    """Three different batches of K windows (every song and several first bars among them)."""
    from style.data import WindowBatch
    rng = np.random.default_rng(K)
    out = []
    for _ in range(3):
        ids = rng.integers(0, len(wc.SONG_BARS), K)
        r0s = [int(rng.integers(0, wc.SONG_BARS[s] - BARS + 1)) for s in ids]
        out.append(WindowBatch(C, BARS, T, True, ids, r0s))
    assert len({(tuple(b.songs), tuple(b.r0s)) for b in out}) == 3
    return out


_planK = {}


def plan_reference(model, batch):
    """K x 15 losses and K x (C + 2) x 8 metrics of the batch from a Plan(clips = K) driven directly on host-cropped dense clips
    with set_inputs per clip (eval_cases._run_eval), as host tensors; and the plan's tiling."""
    from style import _native as nat
    K = batch.K
    if K not in _planK:
        _planK[K] = nat.Plan(_native(), make_dims(pc.SMALL, C, BARS, T, True, clips=K), DEV)
    dense = wc.cropped(batch)
    xp, xu = torch.cat([p for p, _ in dense]).to(DEV), torch.cat([u for _, u in dense]).to(DEV)
    _, losses, metrics = ec._run_eval(_planK[K], model._flat, xp, xu, [wc.songs()[s] for s in batch.songs.tolist()], True)
    torch.cuda.synchronize()
    return losses.cpu(), metrics.cpu(), _planK[K].gemm_tile


@pytest.mark.parametrize('K,tile', [(3, 32), (8, 64)])
def test_eval_windows_equals_the_batched_plan_on_host_cropped_clips(K, tile):
    """Three consecutive calls with different windows of one shape — eager, capture + replay, replay — and a fourth with an
    accumulator (its own capture): each bit-identical, in per-clip losses and metrics, to Plan(clips=K).eval_iteration on the
    host-cropped dense clips.  A padded batch with live = 1 counts one clip.  At K = 3 (the one-clip tiling) the per-clip losses
    are also those of the model's one-clip eval_iteration on the cropped clips, bit for bit — parity_cases.batch_case's property."""
    from style import _native as nat
    model = small_model()
    store = wc.make_store(DEV)
    todo = batches(K)
    plan = model._plan(C, BARS, T, True, torch.device(DEV), clips=K)
    plan.__dict__.pop('_eval_window_state', None)                       # (plans are cached per shape: start from a first use)
    for n, batch in enumerate(todo):
        want_l, want_m, got_tile = plan_reference(model, batch)
        assert got_tile == tile == plan.gemm_tile
        got_l, got_m = model.eval_windows(store, batch)
        torch.cuda.synchronize()
        assert got_l.shape == (K, 15) and got_m.shape == (K, C + 2, 8) and got_m.dtype == torch.float64 and got_l.is_cuda
        assert torch.isfinite(got_l).all()
        assert ec.same_bits(got_l, want_l) and ec.same_bits(got_m, want_m), n
        assert (plan.__dict__['_eval_window_state']['graph'] is not None) == (n >= 1)          # a replay from the second use on
    assert ec.counts_not_trivial(want_m[:, :C].numpy()) and ec.counts_not_trivial(want_m[:, C].numpy())
    # a padded batch into an accumulator: only the first window counts
    from style.data import WindowBatch
    padded = WindowBatch(C, BARS, T, True, [1] * K, [3] * K)
    want_l, want_m, _ = plan_reference(model, padded)
    acc = model.eval_accumulator()
    acc.zero_()
    for rounds in (1, 2):                                               # capture (the accumulator is a new address), then replay
        got_l, got_m = model.eval_windows(store, padded, live=1, acc=acc)
        torch.cuda.synchronize()
        assert ec.same_bits(got_l, want_l) and ec.same_bits(got_m, want_m)
    want = wc.fold(wc.fold(np.zeros(wc.ACC), want_l.numpy(), want_m.numpy(), 1), want_l.numpy(), want_m.numpy(), 1)
    assert wc.same_doubles(acc.cpu().numpy(), want) and want[0] == 2 and want[40] == 2
    assert plan.__dict__['_eval_window_state']['graph'] is not None
    with pytest.raises(nat.MstError):
        model.eval_windows(wc.make_store('cpu'), padded)                # a store on another device is refused
    with pytest.raises(nat.MstError):
        model.eval_windows(store, padded, acc=torch.zeros(41, device=DEV))
    if K == 3:
        batch = todo[0]
        got_l, _ = model.eval_windows(store, batch)
        for k, ((xp, xu), s) in enumerate(zip(wc.cropped(batch), batch.songs.tolist())):
            clip = wc.songs()[s]
            res = model.eval_iteration(clip['mode'].to(DEV), clip['bpm'].to(DEV), xp.to(DEV), clip['instruments_features'].to(DEV),
                                       xu.to(DEV), clip['used_instruments'].to(DEV), clip['bpm_int'])
            assert ec.same_bits(res.losses, got_l[k]), k
    model.check_device_status()


def test_evaluate_windows_is_the_fold_of_its_batches():
    from style.metrics import round_result
    from style.train import evaluate_windows
    model = small_model()
    store = wc.make_store(DEV)
    want = np.zeros(wc.ACC)
    todo = store.window_batches(BARS, 3)
    assert [live for _, live in todo] == [3, 3, 1]
    for batch, live in todo:
        losses, metrics, _ = plan_reference(model, batch)
        want = wc.fold(want, losses.numpy(), metrics.numpy(), live)
    seen = []
    for _ in range(2):                                                  # two rounds: the same bits
        res = evaluate_windows(model, store, BARS, 3)
        seen.append(model.eval_accumulator().cpu().numpy().copy())
        assert wc.same_doubles(seen[-1], want)
        assert res['clips'] == 7 and res['windows_skipped'] == 0
        ref = round_result(want)
        assert wc.same_doubles(res['losses'], ref['losses']) and np.isfinite(res['losses']).all()
        for key in ('pitched', 'unpitched', 'song_info'):
            assert ec.same_bits(res[key].words, ref[key].words)
    assert want[0] == 7 and want[1] == 7 and want[40] == 7              # integer words are exact
    assert want[17] == 7 * C * BARS * T * 560 and want[25] == 7 * BARS * T * 470 and want[33] == 7 * 41
    for at in (17, 25):
        assert all(float(x).is_integer() for x in want[at:at + 5])
    assert 0 < res['pitched'].f1 < 1 and res['song_info'].words[7] == 7
    # another stride is another fixed set
    assert evaluate_windows(model, store, BARS, 3, stride=1)['clips'] == 12


# ---- training is untouched
def test_eval_windows_leaves_the_training_state_alone():
    """Between train_windows and optimizer.step(), and between the two train_iteration calls of an accumulation pair: the
    gradient buffers, the lanes' bookkeeping and the lane counter keep their bits, and train_windows' state is not used."""
    from style.optim import FusedAdam
    store = wc.make_store(DEV)
    train_batch, eval_batch = batches(3)[0], batches(3)[1]
    a = wc.songs()[2]
    feed = lambda clip: (clip['mode'].to(DEV), clip['bpm'].to(DEV), clip['pitched'].to(DEV), clip['instruments_features'].to(DEV),
                         clip['unpitched'].to(DEV), clip['used_instruments'].to(DEV), clip['bpm_int'])
    left = {}
    for with_eval in (False, True):
        model = small_model()
        opt = FusedAdam(model)                                          # switches the two accumulation lanes on
        opt.zero_grad()
        model.train_iteration(*feed(a))                                 # lane 0; the next call would take lane 1
        model.train_windows(store, train_batch)
        if with_eval:
            plan = model._plan(C, BARS, T, True, torch.device(DEV), clips=3)
            torch.cuda.synchronize()
            lanes = model._lane_list
            tw = plan.__dict__['_window_state']
            before = (model._gflat.clone(), lanes[1]['grad'].clone(), model._lane_next, [l['dirty'] for l in lanes], [l['at'] for l in lanes],
                      tw['ws'].clone(), tw['at'], tw['uses'])
            for _ in range(2):                                          # eager, then capture + replay
                losses, _ = model.eval_windows(store, eval_batch, acc=model.eval_accumulator())
            torch.cuda.synchronize()
            assert torch.isfinite(losses).all()
            assert ec.same_bits(model._gflat, before[0]) and ec.same_bits(lanes[1]['grad'], before[1])
            assert (model._lane_next, [l['dirty'] for l in lanes], [l['at'] for l in lanes]) == before[2:5] and model._lane_next == 1
            assert ec.same_bits(tw['ws'], before[5]) and (tw['at'], tw['uses']) == before[6:]
            assert plan.__dict__['_eval_window_state']['ws'].data_ptr() != tw['ws'].data_ptr()
        opt.step()
        torch.cuda.synchronize()
        left[with_eval] = [t.clone() for t in (model._flat, opt.exp_avg, opt.exp_avg_sq, opt.state)]
    for x, y in zip(left[True], left[False]):
        assert ec.same_bits(x, y)
    assert float(left[True][3][0]) == 1


def _driver_songs(first, bars):
    """Small synthetic songs in get_input's form (float64 rolls), as tests/test_gpu_clip_window.py makes them."""
    out = []
    for k, R in enumerate(bars):
        clip = synth_clip(first + k, 2, R, 4, True, density=.03)
        info = dict(bpm=90 + 7 * k, scale=dict(mode='major' if k % 2 else 'minor'))
        out.append((f'song{first + k}', (info, clip['pitched'][0].double().numpy(), clip['instruments_features'][0].double().numpy(),
                                        list(range(2)), clip['unpitched'][0].double().numpy())))
    return out


def test_train_with_windowed_evaluation_rounds(tmp_path):
    from style.metrics import VALIDATION_FIELDS
    from style.train import build_model as build_full, fill_store, train
    held_out = _driver_songs(360, (4, 3, 5, 4))
    expect = fill_store(iter(held_out), 3).windows(2)
    assert len(expect) == 2 + 1 + 2 and expect.skipped == 0                      # the fourth song stays out: eval_windows = 3
    runs = []
    for n, with_eval in enumerate((True, True, False)):
        d = tmp_path / str(n)
        model = build_full(seed=108)
        kwargs = dict(eval_inputs=iter(held_out), eval_every=2, eval_windows=3, eval_info_path=str(d / 'validation.csv')) if with_eval else {}
        with pytest.warns(UserWarning, match='iter_size'):
            train(model, iter(_driver_songs(340, (3, 4, 4, 3, 5))), n_iterations=4, batch_clips=3, window_bars=2, store_songs=4,
                  training_info_path=str(d / 'training.csv'), save_path=None, progress=False, **kwargs)
        torch.cuda.synchronize()
        rows = list(csv.DictReader(open(d / 'validation.csv'))) if with_eval else None
        runs.append((open(d / 'training.csv', 'rb').read(), model._flat.detach().cpu().clone(), rows))
    assert len(runs[0][0]) > 300 and torch.isfinite(runs[0][1]).all()
    for other in runs[1:]:                                              # a second run, and the run without evaluation
        assert runs[0][0] == other[0] and ec.same_bits(runs[0][1], other[1])
    rows = runs[0][2]
    assert rows == runs[1][2]                                           # the validation rows repeat as well
    assert len(rows) == 2 and list(rows[0].keys()) == VALIDATION_FIELDS
    assert [r['iteration'] for r in rows] == ['1', '3'] and all(r['clips'] == str(len(expect)) for r in rows)
    for r in rows:
        assert np.isfinite(float(r['total'])) and float(r['total']) > 0 and r['channels_loss_unpitched_total'] != ''
        assert 0. <= float(r['mode_accuracy']) <= 1.
    assert rows[0] != rows[1]                                           # the parameters moved in between
    for bad in (dict(eval_windows=3), dict(eval_windows=3, eval_inputs=iter(held_out)), dict(eval_windows=3, batch_clips=3),
                dict(eval_windows=0, batch_clips=3, eval_inputs=iter(held_out))):
        with pytest.raises(ValueError):
            train(model, iter(_driver_songs(340, (3, 4))), n_iterations=1, training_info_path=None, save_path=None,
                  progress=False, **bad)
