"""-m gpu: batched style transfer on an MI355X.  mst_clip_gather, mst_rolls_count / mst_rolls_compact and mst_style_sums (the
cases of tests/transfer_cases.py on the gfx950 build) and their composition at the C ABI; StyleTransferModel.transfer_windows
against the batched plan driven from the host (same plan, same input bits: same bits), eager and from its hipGraph, and against
the per-clip Python surface; that training is the same bits with or without it; and style.style_transfer.transfer_songs against
files stitched from the per-clip surface's records."""
import os

import numpy as np
import pytest
import torch

import eval_cases as ec
import eval_window_cases as wc
import parity_cases as pc
import transfer_cases as tc
from simutil import make_dims
from test_gpu_eval_windows import batches, small_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C, T, BARS = wc.C, wc.T, wc.BARS


def _native():
    from style import _native
    return _native.get()


@pytest.mark.parametrize('case', tc.KERNEL_CASES, ids=[c.__name__[5:] for c in tc.KERNEL_CASES])
def test_kernels(case):
    case(_native(), DEV)
    torch.cuda.synchronize()


def test_composition_at_the_c_abi():
    assert tc.case_composition(_native(), DEV, K=3) == 32
    torch.cuda.synchronize()


# ---- StyleTransferModel.transfer_windows
_planK = {}


def plan_reference(model, batch, donors, score):
    """tc.host_reference on a Plan(clips = K) of the model's parameters."""
    from style import _native as nat
    K = batch.K
    if K not in _planK:
        _planK[K] = nat.Plan(_native(), make_dims(pc.SMALL, C, BARS, T, True, clips=K), DEV)
    want = tc.host_reference(_native(), _planK[K], model._flat, batch, donors, DEV, score=score)
    torch.cuda.synchronize()
    return want, _planK[K]


def same_result(got, want, plan, K, score):
    """A TransferResult against tc.host_reference's dict, bit for bit."""
    for name, mine in (('instruments_pred', got.instruments_pred), ('mode_pred', got.mode_pred), ('bpm_pred', got.bpm_pred)):
        ref = torch.stack([plan.view(name, ws=want['ws'], clip=k) for k in range(K)]).reshape(mine.shape)
        assert mine.is_cuda and ec.same_bits(mine, ref) and torch.isfinite(mine).all(), name
    assert got.instruments_pred.shape == (K, 41) and got.mode_pred.shape == (K, 2) and got.bpm_pred.shape == (K,)
    assert len(got.pitched) == len(got.unpitched) == K
    for k in range(K):
        for mine, ref in zip((got.pitched[k], got.unpitched[k]), want['rolls'][k]):
            assert mine.shape == ref.shape and torch.equal(mine.packed, ref.packed), k
            assert 0 < mine.count < mine.n_cells
    if score:
        assert got.style_sums.is_cuda and got.style_sums.dtype == torch.float64 and ec.same_bits(got.style_sums, want['style_sums'])
        assert got.retention.shape == (K, C + 1, 8) and ec.same_bits(got.retention, want['retention'])
    else:
        assert got.style_sums is None and got.retention is None


def donors_of(K, n):
    rng = np.random.default_rng(10 * K + n)
    donors = rng.integers(0, K, K)
    donors[0] = K - 1                                                   # at least one clip takes another's style
    return donors.tolist()


@pytest.mark.parametrize('K,tile', [(3, 32), (8, 64)])
def test_transfer_windows_equals_the_batched_plan_driven_from_the_host(K, tile):
    """Three consecutive calls with different windows and donors of one shape — eager, capture + replay, replay — and a fourth
    with score=True (its own capture): each bit-identical, in song-info predictions, note records and scores, to the same
    Plan(clips=K) driven from the host.  At K = 3 (the one-clip tiling) the records and song-info predictions are also those of
    the per-clip Python surface on the host-cropped clips — parity_cases.batch_case's property."""
    from style import _native as nat
    from style.metrics import style_cosines
    from style.model import hard_output_sparse
    model = small_model()
    store = wc.make_store(DEV)
    todo = batches(K)
    plan = model._plan(C, BARS, T, True, torch.device(DEV), clips=K)
    plan.__dict__.pop('_transfer_window_state', None)                   # (plans are cached per shape: start from a first use)
    for n, batch in enumerate(todo):
        donors = donors_of(K, n)
        want, ref_plan = plan_reference(model, batch, donors, False)
        assert ref_plan.gemm_tile == tile == plan.gemm_tile
        got = model.transfer_windows(store, batch, donors)
        torch.cuda.synchronize()
        same_result(got, want, ref_plan, K, False)
        assert bool(plan.__dict__['_transfer_window_state']['graphs']) == (n >= 1)          # a replay from the second use on
    kept = got.instruments_pred.clone()
    assert len(plan.__dict__['_transfer_window_state']['graphs']) == 1
    for rounds in (1, 2):                                               # capture (score is part of the key), then replay
        donors = donors_of(K, 3)
        want, ref_plan = plan_reference(model, todo[0], donors, True)
        scored = model.transfer_windows(store, todo[0], donors, score=True)
        torch.cuda.synchronize()
        same_result(scored, want, ref_plan, K, True)
    assert len(plan.__dict__['_transfer_window_state']['graphs']) == 2
    assert ec.same_bits(kept, got.instruments_pred)                     # an earlier result is its own
    cos = style_cosines(scored.style_sums)
    assert cos.shape == (K, 3) and np.isfinite(cos).all() and (np.abs(cos) <= 1 + 1e-12).all()
    assert ec.counts_not_trivial(scored.retention[:, :C].cpu().numpy()) and ec.counts_not_trivial(scored.retention[:, C].cpu().numpy())
    # a capacity one below the largest count is an error that names the capacity needed, never a silent drop
    most = max(r.count for r in scored.pitched + scored.unpitched)
    with pytest.raises(nat.MstError, match=f'capacity={most}'):
        model.transfer_windows(store, todo[0], donors, capacity=most - 1)
    again = model.transfer_windows(store, todo[0], donors, capacity=most)
    assert all(torch.equal(a.packed, b.packed) for a, b in zip(again.pitched + again.unpitched, scored.pitched + scored.unpitched))
    with pytest.raises(nat.MstError):
        model.transfer_windows(wc.make_store('cpu'), todo[0], donors)   # a store on another device is refused
    with pytest.raises(ValueError):
        model.transfer_windows(store, todo[0], donors[:-1])
    if K == 3:
        batch, donors = todo[0], donors_of(K, 0)
        got = model.transfer_windows(store, batch, donors)
        clips = [wc.songs()[s] for s in batch.songs.tolist()]
        feed = [(clip['mode'].to(DEV), clip['bpm'].to(DEV), xp.to(DEV), clip['instruments_features'].to(DEV), xu.to(DEV))
                for clip, (xp, xu) in zip(clips, wc.cropped(batch))]
        with torch.no_grad():
            parts = [model.extract_style(*f) for f in feed]
            for k, d in enumerate(donors):
                style, (_, melody, rhythm) = parts[d][0], parts[k]
                ip, mp, bp = model.predict_song_info(style, rhythm)
                xp, xu = model.apply_style(style, melody, rhythm, feed[d][3], True)
                assert ec.same_bits(ip.reshape(-1), got.instruments_pred[k]) and ec.same_bits(mp.reshape(-1), got.mode_pred[k]), k
                assert ec.same_bits(bp.reshape(-1), got.bpm_pred[k:k + 1]), k
                assert torch.equal(hard_output_sparse(xp).packed, got.pitched[k].packed), k
                assert torch.equal(hard_output_sparse(xu).packed, got.unpitched[k].packed), k
    model.check_device_status()


def test_transfer_windows_leaves_the_training_state_alone():
    """tests/test_gpu_eval_windows.py's property with transfer_windows in the middle: between train_windows and optimizer.step(),
    and between the two train_iteration calls of an accumulation pair, the gradient buffers, the lanes' bookkeeping and the
    lane counter keep their bits, and the states of train_windows and eval_windows are not used."""
    from style.optim import FusedAdam
    store = wc.make_store(DEV)
    train_batch, other_batch = batches(3)[0], batches(3)[1]
    a = wc.songs()[2]
    feed = lambda clip: (clip['mode'].to(DEV), clip['bpm'].to(DEV), clip['pitched'].to(DEV), clip['instruments_features'].to(DEV),
                         clip['unpitched'].to(DEV), clip['used_instruments'].to(DEV), clip['bpm_int'])
    left = {}
    for with_transfer in (False, True):
        model = small_model()
        opt = FusedAdam(model)                                          # switches the two accumulation lanes on
        opt.zero_grad()
        model.train_iteration(*feed(a))                                 # lane 0; the next call would take lane 1
        model.train_windows(store, train_batch)
        if with_transfer:
            plan = model._plan(C, BARS, T, True, torch.device(DEV), clips=3)
            model.eval_windows(store, other_batch)
            torch.cuda.synchronize()
            lanes = model._lane_list
            tw, ew = plan.__dict__['_window_state'], plan.__dict__['_eval_window_state']
            before = (model._gflat.clone(), lanes[1]['grad'].clone(), model._lane_next, [l['dirty'] for l in lanes], [l['at'] for l in lanes],
                      tw['ws'].clone(), tw['at'], tw['uses'], ew['ws'].clone(), ew['at'], ew['uses'])
            for score in (False, False, True):                          # eager, capture + replay, another capture
                got = model.transfer_windows(store, other_batch, [1, 2, 0], score=score)
            torch.cuda.synchronize()
            assert torch.isfinite(got.bpm_pred).all() and torch.isfinite(got.style_sums).all()
            assert ec.same_bits(model._gflat, before[0]) and ec.same_bits(lanes[1]['grad'], before[1])
            assert (model._lane_next, [l['dirty'] for l in lanes], [l['at'] for l in lanes]) == before[2:5] and model._lane_next == 1
            assert ec.same_bits(tw['ws'], before[5]) and (tw['at'], tw['uses']) == before[6:8]
            assert ec.same_bits(ew['ws'], before[8]) and (ew['at'], ew['uses']) == before[9:]
            assert len({plan.__dict__[k]['ws'].data_ptr() for k in ('_window_state', '_eval_window_state', '_transfer_window_state')}) == 3
        opt.step()
        torch.cuda.synchronize()
        left[with_transfer] = [t.clone() for t in (model._flat, opt.exp_avg, opt.exp_avg_sq, opt.state)]
    for x, y in zip(left[True], left[False]):
        assert ec.same_bits(x, y)
    assert float(left[True][3][0]) == 1


# ---- the driver
def surface_file(model, composition_path, style_path, bars, path):
    """The file transfer_songs promises, from the per-clip Python surface: per `bars`-bar window of the composition (the last one
    zero-extended) extract_style -> predict_song_info(donor's style, the window's rhythm) -> apply_style(donor's style, the
    window's melody and rhythm, the donor's instruments, percussion) -> hard_output_sparse; stitched, cut, and written with the
    same tempo / mode rule.  style_path=None: every window with its own style."""
    from style import smf, style_transfer as st
    from style.data import prepare_input
    from style.midi_conversion import ChannelConverter
    from style.model import hard_output_sparse
    from style.scales import major_mode, minor_mode
    from style.sparse import crop_bars, stitch_records

    def windows(song_input):
        mode, bpm, pitched, instr, unpitched = prepare_input(song_input)
        R = pitched.shape[2]
        pad = lambda x: torch.cat([x, x.new_zeros(x.shape[:2] + (-R % bars,) + x.shape[3:])], 2)
        pitched, unpitched = pad(pitched), pad(unpitched)
        return R, [(mode, bpm, pitched[:, :, r0:r0 + bars].contiguous(), instr, unpitched[:, :, r0:r0 + bars].contiguous())
                   for r0 in range(0, R, bars)]
    composition = st.get_model_input(composition_path)
    donor = composition if style_path is None else st.get_model_input(style_path)
    R, clips = windows(composition)
    rolls, bpms, modes = [], [], []
    with torch.no_grad():
        donor_clip = windows(donor)[1][0]
        donor_style = model.extract_style(*donor_clip)[0]
        for clip in clips:
            style, melody, rhythm = model.extract_style(*clip)
            style, instr = (style, clip[3]) if style_path is None else (donor_style, donor_clip[3])
            _, mp, bp = model.predict_song_info(style, rhythm)
            xp, xu = model.apply_style(style, melody, rhythm, instr, True)
            rolls.append((hard_output_sparse(xp), hard_output_sparse(xu)))
            bpms.append(float(bp))
            modes.append(mp.reshape(-1).cpu().tolist())
    info = dict(composition[1][0]) if style_path is None else st.combine_info(style_info=donor[1][0], melody_info=composition[1][0])
    info['tempo'] = smf.bpm2tempo(round(float(np.asarray(bpms, dtype=np.float64).mean())))
    info['scale'] = dict(info['scale'], mode=major_mode if int(np.asarray(modes, dtype=np.float64).sum(0).argmax()) == 0 else minor_mode)
    infos, uinfo = st.channel_slots(donor[1][3])
    mid = st.decode_records(ChannelConverter(info), infos[:clips[0][2].shape[1]], crop_bars(stitch_records([p for p, _ in rolls], bars), R),
                            uinfo, crop_bars(stitch_records([u for _, u in rolls], bars), R))
    mid.save(path)
    return [p.count + u.count for p, u in rolls]


def test_transfer_songs_writes_the_files_of_the_per_clip_surface(tmp_path):
    """Two style songs, bars = 2, K = 3, on small synthetic songs written with the project's MIDI writer: the files equal, byte
    for byte, those stitched from the per-clip surface's records; a style song of another bucket is refused."""
    from style import style_transfer as st
    from style.data import included_instruments as programs
    model = small_model()
    composition = tc.write_song(tmp_path / 'tune.mid', 1, 3, programs[:2])
    styles = [tc.write_song(tmp_path / 'first.mid', 2, 4, programs[2:4], bpm=140), tc.write_song(tmp_path / 'second.mid', 3, 3, programs[1:3], bpm=80)]
    assert st.get_model_input(composition)[1][1].shape[:3] == (2, 5, 2)           # five bars: three windows, the last zero-extended
    out = tmp_path / 'out'
    scores = st.transfer_songs(model, composition, styles, str(out), bars=2, K=3, score=True)
    torch.cuda.synchronize()
    names = {None: 'tune (reconstructed).mid', 'first': 'tune (first style).mid', 'second': 'tune (second style).mid'}
    assert sorted(os.listdir(out / 'tune')) == sorted(names.values()) and set(scores) == set(names)
    seen = set()
    for style_name, style_path in zip((None, 'first', 'second'), [None] + styles):
        want = tmp_path / 'want.mid'
        counts = surface_file(model, composition, style_path, 2, str(want))
        assert len(counts) == 3 and min(counts) > 0
        got = (out / 'tune' / names[style_name]).read_bytes()
        assert got == want.read_bytes() and len(got) > 200, style_name
        seen.add(got)
        score = scores[style_name]
        assert score['cosines'].shape == (3,) and np.isfinite(score['cosines']).all()
        assert score['pitched'].word('cells') == 3 * 2 * 2 * 2 * 560 and score['unpitched'].word('cells') == 3 * 2 * 2 * 470
    assert len(seen) == 3                                                          # three styles, three different files
    assert scores[None]['cosines'][0] == scores[None]['cosines'][1] and abs(scores[None]['cosines'][2] - 1) < 1e-12   # own is donor there
    assert st.transfer_songs(model, composition, styles[:1], str(tmp_path / 'plain'), bars=2, K=3) is None
    assert (tmp_path / 'plain' / 'tune' / names['first']).read_bytes() == (out / 'tune' / names['first']).read_bytes()
    solo = tc.write_song(tmp_path / 'solo.mid', 4, 3, programs[:1])
    with pytest.raises(ValueError, match=r'solo.*\(1, 2, True\).*tune.*\(2, 2, True\)'):
        st.transfer_songs(model, composition, [styles[0], solo], str(tmp_path / 'refused'), bars=2, K=3)
    model.check_device_status()
