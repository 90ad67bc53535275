"""-m gpu: the style bank on an MI355X.  mst_style_put, mst_style_mix and mst_info_decide (the cases of tests/style_bank_cases.py
on the gfx950 build) and their chain at the C ABI; StyleTransferModel.encode_styles against the batched plan driven from the host; transfer_styles against
transfer_windows, against the host-driven plan with numpy-mixed styles and against the per-clip Python surface with
select_instruments on the host; that training is the same bits with both in the middle; and transfer_songs' new arguments against
files stitched from the per-clip surface.  Every comparison is bit equality."""
import os

import numpy as np
import pytest
import torch

import eval_cases as ec
import eval_window_cases as wc
import parity_cases as pc
import style_bank_cases as sb
import transfer_cases as tc
from simutil import make_dims
from test_gpu_eval_windows import batches, small_model
from test_gpu_transfer_windows import surface_file

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C, T, BARS = wc.C, wc.T, wc.BARS
_cache = {}


def _native():
    from style import _native
    return _native.get()


@pytest.mark.parametrize('case', sb.KERNEL_CASES, ids=[c.__name__[5:] for c in sb.KERNEL_CASES])
def test_kernels(case):
    case(_native(), DEV)
    torch.cuda.synchronize()


def test_chain_at_the_c_abi():
    assert sb.case_chain(_native(), DEV, K=3) == 32
    torch.cuda.synchronize()


# ---- the songs: those of eval_window_cases and one of another bucket (C = 1)
def solo():
    if 'solo' not in _cache:
        from tools.synth import synth_clip
        _cache['solo'] = synth_clip(400, 1, 3, T, True, density=.05, bpm=93)
    return _cache['solo']


def all_songs():
    return wc.songs() + [solo()]


def ref_plan(channels, K):
    from style import _native as nat
    if (channels, K) not in _cache:
        _cache[channels, K] = nat.Plan(_native(), make_dims(pc.SMALL, channels, BARS, T, True, clips=K), DEV)
    return _cache[channels, K]


def extracted(model, batch):
    """The host-driven Plan(clips = K) after the extract stage on the host-cropped clips: (plan, ws)."""
    from style import _native as nat
    plan = ref_plan(batch.C, batch.K)
    dense = wc.cropped(batch, all_songs())
    xp, xu = torch.cat([p for p, _ in dense]).to(DEV), torch.cat([u for _, u in dense]).to(DEV)
    ws = plan.new_ws()
    ec._poison(plan, ws, True)
    for k, s in enumerate(batch.songs.tolist()):
        ec._set_clip(plan, all_songs()[s], k, ws)
    plan.forward(nat.STAGE_EXTRACT, model._flat, xp, xu, ws=ws)
    return plan, ws


def rendered(model, batch, styles, instruments, live=None):
    """The host statement of transfer_styles: the plan of `extracted` with its style slots overwritten by `styles` (K x style_size
    float32 numpy), the info stage, the decisions of style_bank_cases.decision taken on the host ('each' / 'pooled') or the
    given rows, the apply stage, sparse.compact(..., 'hard') per clip.  Returns dict(ws, plan, rolls, decisions)."""
    from style import _native as nat
    from style.sparse import compact
    plan, ws = extracted(model, batch)
    K, CH = batch.K, batch.C
    for k in range(K):
        plan.view('style', ws=ws, clip=k).copy_(torch.from_numpy(styles[k]))
    plan.forward(nat.STAGE_INFO, model._flat, None, None, ws=ws)
    decisions = None
    if isinstance(instruments, str):
        pred = [[plan.view(n, ws=ws, clip=k).cpu().numpy().reshape(-1) for n in ('instruments_pred', 'mode_pred', 'bpm_pred')] for k in range(K)]
        one = None
        if instruments == 'pooled':
            one = sb.pooled([p[0] for p in pred], [p[1] for p in pred], [p[2][0] for p in pred], K if live is None else live)
        decisions = []
        for k in range(K):
            x, m, b = one if one is not None else (pred[k][0], pred[k][1], pred[k][2][0])
            picks, perc, mode, rows, bpm = sb.decision(x, m, b, CH)
            plan.view('instr', ws=ws, clip=k).copy_(torch.from_numpy(rows.reshape(-1)))
            plan.view('mode', ws=ws, clip=k).copy_(torch.tensor([1. - mode, float(mode)]))
            plan.view('bpm', ws=ws, clip=k).copy_(torch.tensor([float(bpm)]))
            decisions.append(picks + [perc, mode])
    else:
        for k in range(K):
            plan.view('instr', ws=ws, clip=k).copy_(instruments[k if len(instruments) == K else 0].reshape(-1))
    plan.forward(nat.STAGE_APPLY, model._flat, None, None, ws=ws)
    rolls = [(compact(plan.view('pitched_pred', (1, CH, BARS, T, 10, 56, 5), ws=ws, clip=k), 'hard', pin=False, native=_native()),
              compact(plan.view('unpitched_pred', (1, 1, BARS, T, 10, 47, 2), ws=ws, clip=k), 'hard', pin=False, native=_native()))
             for k in range(K)]
    torch.cuda.synchronize()
    return dict(ws=ws, plan=plan, rolls=rolls, decisions=decisions)


def same_as_rendered(got, want, K):
    plan, ws = want['plan'], want['ws']
    for name, mine in (('instruments_pred', got.instruments_pred), ('mode_pred', got.mode_pred), ('bpm_pred', got.bpm_pred),
                       ('instr', got.instr_features)):
        ref = torch.stack([plan.view(name, ws=ws, clip=k) for k in range(K)]).reshape(mine.shape)
        assert mine.is_cuda and ec.same_bits(mine, ref) and torch.isfinite(mine).all(), name
    for k in range(K):
        for mine, ref in zip((got.pitched[k], got.unpitched[k]), want['rolls'][k]):
            assert mine.shape == ref.shape and torch.equal(mine.packed, ref.packed), k
            assert 0 < mine.count < mine.n_cells
    if want['decisions'] is None:
        assert got.decisions is None
    else:
        assert got.decisions.dtype == torch.int32 and got.decisions.cpu().tolist() == want['decisions']


def full_store():
    return wc.make_store(DEV, all_songs())


def bank_of_every_window(model, store, K):
    """Every window of every song (stride 1) in one bank, encoded K at a time — the tiling of the plan that renders, so that a
    window's row is the bits of its own style there —, and {(song, first bar): row}."""
    bank = model.encode_styles(store, BARS, K, stride=1)
    torch.cuda.synchronize()
    return bank, {(song, r0): row for row, (song, r0, bars) in enumerate(bank.provenance)}


def numpy_mix(bank, styles):
    """The numpy loop of float32 products and sums (style_bank_cases.mixed) over the bank's rows: K x style_size float32."""
    offsets, idx, w = bank.mix(styles)
    rows = bank.rows[:len(bank)].cpu().numpy().reshape(-1)
    return np.stack([sb.mixed(rows, len(bank), bank.style_size, offsets, idx, w, k, bank.style_size).view(np.float32)
                     for k in range(len(styles))])


# ---- encode_styles
@pytest.mark.parametrize('K', [3, 8])
def test_encode_styles_fills_the_bank_with_the_plans_style_slots(K):
    """Over a store of two buckets: the bank's rows are, bit for bit, the `style` slots of the same Plan(clips = K) driven from
    the host, batch by batch — the first pass of a plan eager, the second captured, the third replayed (at K = 8 a bucket is one
    batch, so three calls fill one bank).  The repeats that pad a batch take no row, and the provenance names every window."""
    from style.data import StyleBank
    model = small_model()
    store = full_store()
    todo = store.window_batches(BARS, K)
    assert len({b.C for b, _ in todo}) == 2 and any(live < K for _, live in todo)
    for channels in (C, 1):
        model._plan(channels, BARS, T, True, torch.device(DEV), clips=K).__dict__.pop('_encode_style_state', None)
    calls = 1 if K == 3 else 3
    bank = StyleBank(pc.SMALL['style'], DEV, capacity=2 if K == 3 else 32)       # (2: it grows before the first batch, not between)
    for _ in range(calls):
        assert model.encode_styles(store, BARS, K, bank=bank) is bank
    torch.cuda.synchronize()
    windows = [(s, r0) for b, live in todo for s, r0 in zip(b.songs.tolist()[:live], b.r0s.tolist()[:live])]
    assert len(windows) == len(store.windows(BARS)) == 8 and len(bank) == calls * len(windows)
    assert bank.provenance == [(s, r0, BARS) for s, r0 in windows] * calls
    assert bank.by_song[5] == [r for r, p in enumerate(bank.provenance) if p[0] == 5] and len(bank.by_song[1]) == 2 * calls
    rows = bank.rows[:len(bank)].cpu()
    at = 0
    for _ in range(calls):
        for batch, live in todo:
            plan, ws = extracted(model, batch)
            for k in range(live):
                assert ec.same_bits(rows[at], plan.view('style', ws=ws, clip=k).cpu()), (at, k)
                at += 1
    assert at == len(bank) and torch.isfinite(rows).all() and len({bytes(tc.words(r)) for r in rows[:len(windows)]}) == len(windows)
    assert (bank.rows[len(bank):] == 0).all()                            # nothing beyond the rows taken
    for channels in (C, 1):
        st = model._plan(channels, BARS, T, True, torch.device(DEV), clips=K).__dict__['_encode_style_state']
        assert (st['graph'] is not None) == (st['uses'] >= 2)
    assert model._plan(C, BARS, T, True, torch.device(DEV), clips=K).__dict__['_encode_style_state']['graph'] is not None
    with pytest.raises(Exception):
        model.encode_styles(wc.make_store('cpu'), BARS, K)
    model.check_device_status()


# ---- transfer_styles
@pytest.mark.parametrize('K', [3, 8])
def test_transfer_styles_with_one_row_each_is_transfer_windows(K):
    """The mix is one weight-1 entry per clip, the bank row of clip donors[k]'s window, and the instruments are the donors' rows:
    song-info predictions and note records are transfer_windows(store, batch, donors)'s, bit for bit — eager, captured, replayed."""
    model = small_model()
    store = full_store()
    bank, row_of = bank_of_every_window(model, store, K)
    plan = model._plan(C, BARS, T, True, torch.device(DEV), clips=K)
    plan.__dict__.pop('_transfer_style_state', None)
    for n, batch in enumerate(batches(K)):
        donors = np.random.default_rng(7 * K + n).integers(0, K, K).tolist()
        donors[0] = K - 1
        want = model.transfer_windows(store, batch, donors)
        songs, r0s = batch.songs.tolist(), batch.r0s.tolist()
        mix = [bank.row(row_of[songs[d], r0s[d]]) for d in donors]
        instr = torch.cat([wc.songs()[songs[d]]['instruments_features'] for d in donors])
        got = model.transfer_styles(store, batch, bank, bank.mix(mix) if n else mix, instruments=instr)
        torch.cuda.synchronize()
        for name in ('instruments_pred', 'mode_pred', 'bpm_pred'):
            assert ec.same_bits(getattr(got, name), getattr(want, name)) and torch.isfinite(getattr(got, name)).all(), (name, n)
        for k in range(K):
            assert torch.equal(got.pitched[k].packed, want.pitched[k].packed) and torch.equal(got.unpitched[k].packed, want.unpitched[k].packed)
            assert 0 < got.pitched[k].count < got.pitched[k].n_cells
        assert got.decisions is None and ec.same_bits(got.instr_features, instr.to(DEV)) and got.style_sums is None
        states = plan.__dict__['_transfer_style_state']
        assert list(states) == [4 * K] and bool(states[4 * K]['graphs']) == (n >= 1)
    model.check_device_status()


def test_transfer_styles_blends_decides_and_crosses_buckets():
    """K = 3, the one-clip tiling.  Clip 0 takes the style of a window of the C = 1 song, clip 1 a blend of two songs' means, clip
    2 the mean of a song.  With 'each' the result is the host-driven plan's with the numpy mix in its style slots, and the per-clip
    Python surface's with select_instruments on the host; with 'pooled' (live = 2) and with given rows it is the host-driven
    plan's; with score the side buffer's sums are the host's float64 loops.  More entries than a state holds open another."""
    from style.data import _instrument_categories, encode_instruments
    from style.model import hard_output_sparse
    from style.style_transfer import select_instruments
    K = 3
    model = small_model()
    store = full_store()
    bank, row_of = bank_of_every_window(model, store, K)
    plan = model._plan(C, BARS, T, True, torch.device(DEV), clips=K)
    plan.__dict__.pop('_transfer_style_state', None)
    batch = batches(K)[0]
    styles = [bank.row(row_of[5, 1]), bank.blend([(1, .5), (3, .5)]), bank.song(4)]
    assert [len(s) for s in styles] == [1, 4 + 3, 2]
    mixed = numpy_mix(bank, styles)
    assert ec.same_bits(torch.from_numpy(mixed[0]), bank.rows[row_of[5, 1]].cpu())       # one entry of weight 1: the row's bits
    for n in range(3):                                                   # eager, captured, replayed
        got = model.transfer_styles(store, batch, bank, styles, instruments='each')
        torch.cuda.synchronize()
        want = rendered(model, batch, mixed, 'each')
        same_as_rendered(got, want, K)
    own = model.transfer_windows(store, batch, [0, 1, 2])
    assert not ec.same_bits(own.instruments_pred[0], got.instruments_pred[0])            # the foreign style matters
    # the per-clip Python surface
    clips = [wc.songs()[s] for s in batch.songs.tolist()]
    with torch.no_grad():
        for k, (clip, (xp, xu)) in enumerate(zip(clips, wc.cropped(batch))):
            _, melody, rhythm = model.extract_style(clip['mode'].to(DEV), clip['bpm'].to(DEV), xp.to(DEV), clip['instruments_features'].to(DEV),
                                                    xu.to(DEV))
            style = torch.from_numpy(mixed[k]).to(DEV).reshape(1, -1)
            ip, mp, bp = model.predict_song_info(style, rhythm)
            programs, _ = select_instruments(ip.cpu().numpy()[0], C + 1)
            feats = torch.tensor(encode_instruments(programs[:C]), dtype=torch.float).to(DEV).unsqueeze(0)
            yp, yu = model.apply_style(style, melody, rhythm, feats, True)
            assert ec.same_bits(ip.reshape(-1), got.instruments_pred[k]) and ec.same_bits(mp.reshape(-1), got.mode_pred[k]), k
            assert ec.same_bits(bp.reshape(-1), got.bpm_pred[k:k + 1]) and ec.same_bits(feats[0], got.instr_features[k]), k
            assert [_instrument_categories[i] for i in got.decisions[k, :C].tolist()] == programs[:C]
            assert torch.equal(hard_output_sparse(yp).packed, got.pitched[k].packed), k
            assert torch.equal(hard_output_sparse(yu).packed, got.unpitched[k].packed), k
    # pooled, and given rows (one for all, one each)
    got = model.transfer_styles(store, batch, bank, styles, instruments='pooled', live=2)
    same_as_rendered(got, rendered(model, batch, mixed, 'pooled', live=2), K)
    assert ec.same_bits(got.instr_features[0], got.instr_features[2]) and (got.decisions == got.decisions[0]).all()
    for rows in (clips[1]['instruments_features'], torch.cat([c['instruments_features'] for c in clips[::-1]])):
        got = model.transfer_styles(store, batch, bank, styles, instruments=rows)
        same_as_rendered(got, rendered(model, batch, mixed, rows.to(DEV)), K)
    states = plan.__dict__['_transfer_style_state']
    assert list(states) == [4 * K] and len(states[4 * K]['graphs']) == 4                 # each, pooled, given x 1, given x K
    # the score: own styles in rows [0, K) of the side buffer, the mixed targets in [K, 2 K)
    scored = model.transfer_styles(store, batch, bank, styles, instruments='each', score=True)
    torch.cuda.synchronize()
    sums = scored.style_sums.cpu().numpy()
    songs, r0s = batch.songs.tolist(), batch.r0s.tolist()
    for k in range(K):
        mine = bank.rows[row_of[songs[k], r0s[k]]].cpu().numpy()
        want = [tc.dot(mixed[k], mixed[k]), tc.dot(mine, mine), tc.dot(mixed[k], mine)]
        assert np.array_equal(sums[k, [1, 2, 5]].view(np.uint64), np.asarray(want).view(np.uint64)), k
    assert np.isfinite(scored.cosines).all() and scored.retention.shape == (K, C + 1, 8)
    assert all(torch.equal(a.packed, b.packed) for a, b in zip(scored.pitched, want_rolls(model, batch, mixed)))
    # 16 entries do not fit a state of 4 K = 12: another state, the same arithmetic
    many = [bank.blend([(1, .25), (3, .25), (4, .25), (0, .25)]) + bank.row(0) * 4, bank.row(1), bank.row(2)]
    assert sum(len(s) for s in many) == 16
    got = model.transfer_styles(store, batch, bank, many, instruments='each')
    same_as_rendered(got, rendered(model, batch, numpy_mix(bank, many), 'each'), K)
    assert sorted(states) == [4 * K, 8 * K]
    # a clip without entries, or with a row outside the bank, is NaN in its predictions only
    got = model.transfer_styles(store, batch, bank, [bank.row(0), [], [(bank.capacity, np.float32(1.))]], instruments='each')
    assert torch.isfinite(got.instruments_pred[0]).all() and torch.isnan(got.instruments_pred[1:]).all()
    with pytest.raises(ValueError):
        model.transfer_styles(store, batch, bank, styles[:2])
    with pytest.raises(ValueError):
        model.transfer_styles(store, batch, bank, styles, instruments='donor')
    model.check_device_status()


def want_rolls(model, batch, mixed):
    return [p for p, _ in rendered(model, batch, mixed, 'each')['rolls']]


def test_encode_and_transfer_styles_leave_the_training_state_alone():
    """test_transfer_windows_leaves_the_training_state_alone's property with encode_styles and transfer_styles in the middle:
    between train_windows and optimizer.step() the gradient buffers, the lanes' bookkeeping, the lane counter and the states of
    train_windows, eval_windows and transfer_windows keep their bits, and the optimizer's step is the same bits."""
    from style.optim import FusedAdam
    store = wc.make_store(DEV)
    train_batch, other_batch = batches(3)[0], batches(3)[1]
    a = wc.songs()[2]
    feed = lambda clip: (clip['mode'].to(DEV), clip['bpm'].to(DEV), clip['pitched'].to(DEV), clip['instruments_features'].to(DEV),
                         clip['unpitched'].to(DEV), clip['used_instruments'].to(DEV), clip['bpm_int'])
    left = {}
    for with_styles in (False, True):
        model = small_model()
        opt = FusedAdam(model)                                          # switches the two accumulation lanes on
        opt.zero_grad()
        model.train_iteration(*feed(a))                                 # lane 0; the next call would take lane 1
        model.train_windows(store, train_batch)
        if with_styles:
            plan = model._plan(C, BARS, T, True, torch.device(DEV), clips=3)
            model.eval_windows(store, other_batch)
            model.transfer_windows(store, other_batch, [1, 2, 0])
            torch.cuda.synchronize()
            lanes = model._lane_list
            keys = ('_window_state', '_eval_window_state', '_transfer_window_state')
            states = [plan.__dict__[k] for k in keys]
            before = (model._gflat.clone(), lanes[1]['grad'].clone(), model._lane_next, [l['dirty'] for l in lanes], [l['at'] for l in lanes],
                      [s['ws'].clone() for s in states], [(s['at'], s['uses']) for s in states])
            bank = model.encode_styles(store, BARS, 3)
            bank = model.encode_styles(store, BARS, 3, bank=bank)       # captures and replays
            for score in (False, False, True):                          # eager, capture + replay, another capture
                got = model.transfer_styles(store, other_batch, bank, [bank.song(0), bank.song(1), bank.row(3)], 'pooled', score=score)
            torch.cuda.synchronize()
            assert torch.isfinite(got.bpm_pred).all() and torch.isfinite(got.style_sums).all() and torch.isfinite(bank.rows).all()
            assert ec.same_bits(model._gflat, before[0]) and ec.same_bits(lanes[1]['grad'], before[1])
            assert (model._lane_next, [l['dirty'] for l in lanes], [l['at'] for l in lanes]) == before[2:5] and model._lane_next == 1
            for s, ws, counters in zip(states, before[5], before[6]):
                assert ec.same_bits(s['ws'], ws) and (s['at'], s['uses']) == counters
            mine = [plan.__dict__['_encode_style_state'], *plan.__dict__['_transfer_style_state'].values()]
            assert len({s['ws'].data_ptr() for s in states + mine}) == len(states) + len(mine)
        opt.step()
        torch.cuda.synchronize()
        left[with_styles] = [t.clone() for t in (model._flat, opt.exp_avg, opt.exp_avg_sq, opt.state)]
    for x, y in zip(left[True], left[False]):
        assert ec.same_bits(x, y)
    assert float(left[True][3][0]) == 1


# ---- the driver
def predicted_file(model, composition_path, style_path, bars, K, path):
    """The file transfer_songs(song_styles=True, instruments='predicted') promises, from the per-clip Python surface: the style is
    the float32 mean (the weights float32(1) / float32(n), products and sums in window order) of extract_style over the style
    song's full, sounding windows (SongStore.windows); per composition window predict_song_info(style, the window's rhythm); ONE decision — the device's rule on
    the fp32 sums of the predictions of the first K windows — whose instruments every window plays; stitched, cut and written with
    transfer_songs' tempo / mode rule and the decided programs."""
    from style import smf, style_transfer as st
    from style.data import _instrument_categories, prepare_input
    from style.midi_conversion import ChannelConverter
    from style.model import hard_output_sparse
    from style.scales import major_mode, minor_mode
    from style.sparse import crop_bars, stitch_records

    def windows(song_input, full_only):
        mode, bpm, pitched, instr, unpitched = prepare_input(song_input)
        R = pitched.shape[2]
        pad = lambda x: torch.cat([x, x.new_zeros(x.shape[:2] + (-R % bars,) + x.shape[3:])], 2)
        pitched, unpitched = pad(pitched), pad(unpitched)
        return R, [(mode, bpm, pitched[:, :, r0:r0 + bars].contiguous(), instr, unpitched[:, :, r0:r0 + bars].contiguous())
                   for r0 in range(0, R - bars + 1 if full_only else R, bars)]
    composition, donor = st.get_model_input(composition_path), st.get_model_input(style_path)
    R, clips = windows(composition, False)
    channels = clips[0][2].shape[1]
    with torch.no_grad():
        sounds = lambda clip: bool((clip[2] != 0).any()) and bool((clip[4] != 0).any())       # SongStore.window_sounds' rule
        donor_windows = [clip for clip in windows(donor, True)[1] if sounds(clip)]
        assert 1 < len(donor_windows) < len(windows(donor, True)[1])                       # (the song's last window is silent)
        donor_styles = [model.extract_style(*clip)[0].cpu().numpy().reshape(-1) for clip in donor_windows]
        w = np.float32(1.) / np.float32(len(donor_styles))
        style = w * donor_styles[0]
        for x in donor_styles[1:]:
            style = style + w * x
        assert style.dtype == np.float32 and len(donor_styles) > 1
        style = torch.from_numpy(style).to(DEV).reshape(1, -1)
        parts = [model.extract_style(*clip) for clip in clips]
        infos = [[t.cpu().numpy().reshape(-1) for t in model.predict_song_info(style, rhythm)] for _, _, rhythm in parts]
        first = infos[:K]
        picks, _, _, rows, _ = sb.decision(*sb.pooled([i[0] for i in first], [i[1] for i in first], [i[2][0] for i in first], len(first)), channels)
        feats = torch.from_numpy(rows).to(DEV).unsqueeze(0)
        rolls = []
        for _, melody, rhythm in parts:
            xp, xu = model.apply_style(style, melody, rhythm, feats, True)
            rolls.append((hard_output_sparse(xp), hard_output_sparse(xu)))
    info = st.combine_info(style_info=donor[1][0], melody_info=composition[1][0])
    info['tempo'] = smf.bpm2tempo(round(float(np.asarray([float(i[2][0]) for i in infos], dtype=np.float64).mean())))
    modes = np.asarray([i[1].tolist() for i in infos], dtype=np.float64).sum(0)
    info['scale'] = dict(info['scale'], mode=major_mode if int(modes.argmax()) == 0 else minor_mode)
    slots, uinfo = st.channel_slots([_instrument_categories[i] for i in picks])
    mid = st.decode_records(ChannelConverter(info), slots[:channels], crop_bars(stitch_records([p for p, _ in rolls], bars), R),
                            uinfo, crop_bars(stitch_records([u for _, u in rolls], bars), R))
    mid.save(path)
    return [_instrument_categories[i] for i in picks]


def test_transfer_songs_through_the_bank(tmp_path):
    """Default arguments still write the per-clip surface's files.  song_styles=True with instruments='predicted' accepts a C = 1
    style song and writes the file stitched from the per-clip surface with the mean style and one pooled decision (K = 2: the
    composition's three windows are two batches, the second reusing the first's instruments).  A blend of weight 1 on one song
    is that song's own file; a genuine blend is another file."""
    from style import style_transfer as st
    from style.data import included_instruments as programs
    model = small_model()
    composition = tc.write_song(tmp_path / 'tune.mid', 1, 3, programs[:2])
    first = tc.write_song(tmp_path / 'first.mid', 2, 4, programs[2:4], bpm=140)
    second = tc.write_song(tmp_path / 'second.mid', 3, 4, programs[1:3], bpm=80)
    solo_path = tc.write_song(tmp_path / 'solo.mid', 4, 4, programs[:1])
    want = tmp_path / 'want.mid'
    # the defaults: today's files
    st.transfer_songs(model, composition, [first], str(tmp_path / 'plain'), bars=2, K=3)
    surface_file(model, composition, first, 2, str(want))
    plain = (tmp_path / 'plain' / 'tune' / 'tune (first style).mid').read_bytes()
    assert plain == want.read_bytes() and len(plain) > 200
    # the mean style of a song of another bucket, the instruments predicted once
    shape = st.get_model_input(solo_path)[1][1].shape
    assert shape[0] == 1 and shape[1] >= 4 and shape[2] == 2        # another bucket, and more than one full window
    st.transfer_songs(model, composition, [solo_path], str(tmp_path / 'mean'), bars=2, K=2, song_styles=True, instruments='predicted')
    torch.cuda.synchronize()
    picked = predicted_file(model, composition, solo_path, 2, 2, str(want))
    got = (tmp_path / 'mean' / 'tune' / 'tune (solo style).mid').read_bytes()
    assert got == want.read_bytes() and len(got) > 200 and len(picked) == 2
    assert sorted(os.listdir(tmp_path / 'mean' / 'tune')) == ['tune (reconstructed).mid', 'tune (solo style).mid']
    with pytest.raises(ValueError, match=r'solo.*\(1, 2, True\).*tune.*\(2, 2, True\)'):
        st.transfer_songs(model, composition, [solo_path], str(tmp_path / 'refused'), bars=2, K=2, song_styles=True)
    # blends
    blends = [{'name': 'only', 'parts': {'second': 1.}}, {'name': 'half', 'parts': {'first': .5, 'second': .5}}]
    scores = st.transfer_songs(model, composition, [first, second], str(tmp_path / 'blend'), bars=2, K=3, score=True, song_styles=True, blends=blends)
    out = tmp_path / 'blend' / 'tune'
    assert sorted(os.listdir(out)) == sorted(f'tune ({n}).mid' for n in ('reconstructed', 'first style', 'second style', 'only style', 'half style'))
    files = {n: (out / f'tune ({n} style).mid').read_bytes() for n in ('first', 'second', 'only', 'half')}
    assert files['only'] == files['second'] and len({files['first'], files['second'], files['half']}) == 3
    assert set(scores) == {None, 'first', 'second', 'only', 'half'} and all(np.isfinite(s['cosines']).all() for s in scores.values())
    with pytest.raises(ValueError):
        st.transfer_songs(model, composition, [first], str(tmp_path / 'bad'), bars=2, K=3, blends=[{'name': 'x', 'parts': {'second': 1.}}])
    model.check_device_status()
