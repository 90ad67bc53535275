"""Style transfer between MIDI songs: the reference's inference driver (style/style_transfer.py:22-158)
over the HIP model.  Forward only, one pass per song:

    composition.mid --extract_style--> (style_A, melody_A, rhythm_A)
    style_k.mid     --extract_style--> style_k
    apply_style(style_k, melody_A, rhythm_A) --hard_output--> piano-rolls --> MIDI

The per-song host decisions are split out so they can be tested without a GPU:
`select_instruments` (top-n programs out of the 41 predicted logits, :105-116), `combine_info` (:134-142)
and `decode_rolls` (rolls -> MidiFile, the host half of `decode_midi`).  With `sparse_output=True` the dense
hard rolls never reach the host: `hard_output_sparse` compacts them to note records on the GPU and
`decode_records` writes the same file from those, byte for byte.  Behaviour kept from the
reference: songs are cut to `1000 // C` bars for the encoder (:69) while `original/*.mid` is written
from the full-length rolls; `apply_style` overwrites `info['tempo']` and `info['scale']['mode']` of the
dict it is given (the scale dict is shared with the style song's info); an existing output directory is
never cleared (the reference's `shutil.rmtree` raises NameError inside a bare `except`, :31-34).
"""
import os

import numpy as np
import torch

from style import smf
from style.data import (included_instruments, get_input, prepare_input, percussion_id, encode_instruments,
                        _instrument_categories)
from style.midi import load_midi_from_file, create_midi
from style.midi_conversion import ChannelConverter, read_midi
from style.model import device, hard_output, hard_output_sparse
from style.scales import major_mode, minor_mode


def transfer_style(model, composition_path, style_paths, output_path, sparse_output=False):
    composition_name = os.path.splitext(os.path.basename(composition_path))[0]
    composition_input = get_model_input(composition_path)
    _, (composition_info, composition_pitched, _, composition_instruments, composition_unpitched) = composition_input
    composition_cc = ChannelConverter(composition_info)
    style_, melody, rhythm = extract_style(model, composition_input)
    output_path = os.path.join(output_path, composition_name)

    save(composition_cc, composition_pitched, composition_unpitched, composition_instruments,
         os.path.join(output_path, f'original/{composition_name}.mid'), sparse_output=sparse_output)
    apply_style(model, composition_info, style_, melody, rhythm, len(composition_instruments),
                os.path.join(output_path, f'{composition_name} (reconstructed).mid'), sparse_output=sparse_output)
    for style_path in style_paths:
        style_name = os.path.splitext(os.path.basename(style_path))[0]
        style_input = get_model_input(style_path)
        _, (style_info, style_pitched, _, style_instruments, style_unpitched) = style_input
        style, _, _ = extract_style(model, style_input)
        save(ChannelConverter(style_info), style_pitched, style_unpitched, style_instruments,
             os.path.join(output_path, f'original/{style_name}.mid'), sparse_output=sparse_output)
        info = combine_info(style_info=style_info, melody_info=composition_info)
        apply_style(model, info, style, melody, rhythm, len(style_instruments),
                    os.path.join(output_path, f'{composition_name} ({style_name} style).mid'), sparse_output=sparse_output)


def transfer_songs(model, composition_path, style_paths, output_path, bars=16, K=8, score=False, song_styles=False, blends=(),
                   instruments='donor', library=None, nearest=0):
    """`transfer_style` on resident songs, K windows per pass (StyleTransferModel.transfer_windows): the composition and the
    style songs are loaded as `transfer_style` loads them, kept in a SongStore on the model's device, and for every style song
    the composition's consecutive `bars`-bar windows (the last one zero-extended) are rendered with the style and the
    instruments of the style song's window at bar 0.  A batch holds K - 1 composition windows and that donor window, which
    every donor index points at; the last batch repeats its last window, and the repeats are ignored.  The windows' note
    records are stitched, cut to the composition's bars and written with `decode_records` as
    '{composition} ({style} style).mid' — and, rendered with each window's own style, '{composition} (reconstructed).mid' —
    under output_path/{composition}, with the donor's programs (`channel_slots`), the tempo
    smf.bpm2tempo(round(mean of bpm_pred over the windows)) and the mode of the largest summed mode_pred, as `apply_style`
    derives both for one clip.  Unlike `apply_style` the instruments are the donor's own, not the top picks of
    instruments_pred.  A style song of another (channels, beats per bar, percussion) bucket than the composition's cannot share
    its batched plan: ValueError naming both (`transfer_style` remains for those).

    With `score` it returns {style name: dict(cosines=the mean over the windows of style.metrics.style_cosines — rendered
    against donor, rendered against own, own against donor —, pitched=, unpitched= the summed note-retention NoteMetrics)},
    the reconstruction under the key None; else None.

    `song_styles`, `blends` and `instruments` lift those limits through a style bank (StyleTransferModel.encode_styles /
    transfer_styles); with their defaults nothing above changes.  Every song is then encoded once — its full, sounding
    `bars`-bar windows at stride `bars` (SongStore.windows) — and a batch holds K composition windows.
    song_styles=True: a style song's style is the mean of its windows instead of its window at bar 0.
    blends=[{'name': 'half', 'parts': {'first': .5, 'second': .5}}]: besides the style songs' files, '{composition} (half
    style).mid' rendered with the weighted sum of the named style songs' styles; scale, donor instruments and style name are
    those of its first part.
    instruments='predicted': the clips play what the model predicts, not the donor's programs — apply_style's rule, decided on
    the device (mst_info_decide) once per file, on the predictions summed over the live windows of the file's first batch; the
    later batches reuse that batch's instrument rows, and the programs written are the decided ones.  The donor's instrument
    rows are then not needed, so a style song of another bucket than the composition's is accepted.

    library=a style.data.StyleBank on the model's device or the path of one saved with StyleBank.save, nearest=k > 0: besides
    the files above, '{composition} (library style).mid', every composition window rendered with the uniform blend of the k
    rows of the library nearest to the window's own style by cosine (StyleTransferModel.transfer_styles with
    style.data.Nearest(k, exclude_own=False): searched, mixed and rendered on the device).  A library has no donor instrument
    rows, so the instruments are the 'predicted' ones, and scale and style name are the composition's.  The call then returns
    the result dict also without `score`, with the picked rows' provenance under the key 'library' — per composition window the
    k (song, first bar, bars) — and with `score` the file's scores under 'library style'."""
    from style.data import Nearest, SongStore, StyleBank, WindowBatch, prepare_input_sparse
    from style.metrics import NoteMetrics, style_cosines
    from style.sparse import crop_bars, stitch_records
    bars, K, nearest = int(bars), int(K), int(nearest)
    if bars < 1 or K < 2:
        raise ValueError('transfer_songs: bars >= 1, and K >= 2 (a batch holds the donor window and at least one other)')
    if nearest < 0 or (nearest > 0 and library is None):
        raise ValueError(f'transfer_songs: nearest = {nearest} needs nearest >= 0 and, above 0, a library')
    play = instruments
    if play not in ('donor', 'predicted'):
        raise ValueError(f"transfer_songs: instruments is 'donor' or 'predicted', not {play!r}")
    through_bank = bool(song_styles) or bool(blends) or play == 'predicted'
    name_of = lambda path: os.path.splitext(os.path.basename(path))[0]
    composition_name = name_of(composition_path)
    store = SongStore(next(model.parameters()).device)
    jobs = []
    for path in [composition_path] + list(style_paths):
        song_input = get_model_input(path)
        _, (info, _, _, instruments, _) = song_input
        song = store.add(prepare_input_sparse(song_input))
        if store.bucket_of(song) != store.bucket_of(0) and play != 'predicted':
            raise ValueError(f'{name_of(path)} is of the (channels, beats per bar, percussion) bucket {store.bucket_of(song)}, '
                             f'{composition_name} of {store.bucket_of(0)}: they cannot share a batch; use transfer_style')
        jobs.append((song, info, instruments, None if song == 0 else name_of(path)))
    composition_info = jobs[0][1]
    C, T, U = store.bucket_of(0)
    R = store.songs[0]['R']
    starts = list(range(0, R, bars))
    output_path = os.path.join(output_path, composition_name)
    os.makedirs(output_path, exist_ok=True)
    scores = {}
    if through_bank:
        bank = model.encode_styles(store, bars, K)

        def style_of(song):
            rows = bank.by_song.get(song, [])
            first = [r for r in rows if bank.provenance[r][1] == 0]
            if not rows or not (song_styles or first):
                raise ValueError(f'transfer_songs: {jobs[song][3]} has no full, sounding window of {bars} bars to take a style from')
            return bank.song(song) if song_styles else bank.row(first[0])
        by_name = {job[3]: job for job in jobs[1:]}
        todo = [(job, style_of(job[0]), job[3]) for job in jobs[1:]]
        for blend in blends:
            parts = list(blend['parts'].items())
            missing = [name for name, _ in parts if name not in by_name]
            if missing or not parts:
                raise ValueError(f'transfer_songs: the blend {blend["name"]!r} names {missing or "no style song"}')
            todo.append((by_name[parts[0][0]], bank.blend([(style_of(by_name[name][0]), weight) for name, weight in parts]), blend['name']))
        for (song, song_info, donor_programs, _), entries, style_name in todo:
            if play == 'donor' and store.bucket_of(song) != store.bucket_of(0):
                raise ValueError(f'{style_name}: donor instruments need a style song of the bucket {store.bucket_of(0)}')
            got, rows = [], None
            if play == 'donor':
                rows = torch.tensor(encode_instruments(donor_programs)[:C], dtype=torch.float).unsqueeze(0)
            for at in range(0, len(starts), K):
                part = starts[at:at + K]
                live = len(part)
                batch = WindowBatch(C, bars, T, U, [0] * K, part + [part[-1]] * (K - live))
                res = model.transfer_styles(store, batch, bank, [entries] * K, instruments='pooled' if rows is None else rows, score=score,
                                            live=live)
                if rows is None:                                # the file's one decision: the later batches play the same
                    rows, picked = res.instr_features[:1].clone(), res.decisions[0, :C].cpu().tolist()
                    donor_programs = [_instrument_categories[i] for i in picked]
                got.append((res, live))
            scores[style_name] = _write_transfer(got, composition_info, song_info, donor_programs, C, R, U, bars, score,
                                                 os.path.join(output_path, f'{composition_name} ({style_name} style).mid'))
        jobs = jobs[:1]                                         # the reconstruction is transfer_windows', as ever
    if nearest > 0:
        if not isinstance(library, StyleBank):
            library = StyleBank.load(library, store.device)
        got, rows, picks = [], None, []
        for at in range(0, len(starts), K):
            part = starts[at:at + K]
            live = len(part)
            batch = WindowBatch(C, bars, T, U, [0] * K, part + [part[-1]] * (K - live))
            res = model.transfer_styles(store, batch, library, Nearest(nearest, exclude_own=False), instruments='pooled' if rows is None else rows,
                                        score=score, live=live)
            if rows is None:                                    # the file's one decision, as for instruments='predicted'
                rows, picked = res.instr_features[:1].clone(), res.decisions[0, :C].cpu().tolist()
                programs = [_instrument_categories[i] for i in picked]
            picks += [[library.provenance[r] for r in window] for window in res.neighbours[:live].cpu().tolist()]
            got.append((res, live))
        scored = _write_transfer(got, composition_info, composition_info, programs, C, R, U, bars, score,
                                 os.path.join(output_path, f'{composition_name} (library style).mid'))
        scores['library'] = picks
        if score:
            scores['library style'] = scored
    for song, song_info, instruments, style_name in jobs:
        got = []
        for at in range(0, len(starts), K - 1):
            part = starts[at:at + K - 1]
            live = len(part)
            part = part + [part[-1]] * (K - 1 - live)
            batch = WindowBatch(C, bars, T, U, [0] * (K - 1) + [song], part + [0])
            got.append((model.transfer_windows(store, batch, list(range(K)) if song == 0 else [K - 1] * K, score=score), live))
        each = lambda pick: [x for res, live in got for x in pick(res)[:live]]
        bpm = np.asarray(each(lambda res: res.bpm_pred.cpu().tolist()), dtype=np.float64)
        mode = np.asarray(each(lambda res: res.mode_pred.cpu().tolist()), dtype=np.float64).sum(0)
        info = dict(composition_info) if song == 0 else combine_info(style_info=song_info, melody_info=composition_info)
        info['tempo'] = smf.bpm2tempo(round(float(bpm.mean())))
        info['scale'] = dict(info['scale'], mode=major_mode if int(mode.argmax()) == 0 else minor_mode)
        pitched = crop_bars(stitch_records(each(lambda res: res.pitched), bars), R)
        unpitched = crop_bars(stitch_records(each(lambda res: res.unpitched), bars), R) if U else None
        channels_info, unpitched_info = channel_slots(instruments)
        mid = decode_records(ChannelConverter(info), channels_info[:C], pitched, unpitched_info if U else None, unpitched)
        mid.save(os.path.join(output_path, f'{composition_name} (reconstructed).mid' if song == 0 else
                              f'{composition_name} ({style_name} style).mid'))
        if score:
            retention = torch.cat([res.retention[:live] for res, live in got]).cpu()
            scores[style_name] = dict(cosines=np.concatenate([style_cosines(res.style_sums)[:live] for res, live in got]).mean(0),
                                      pitched=NoteMetrics(retention[:, :-1]).sum(), unpitched=NoteMetrics(retention[:, -1]).sum())
    return scores if score or nearest > 0 else None


def _write_transfer(got, composition_info, style_info, programs, C, R, U, bars, score, path):
    """The file of one style from the batches' results [(TransferResult, live)], by transfer_songs' rules: the tempo of the mean
    bpm_pred, the mode of the summed mode_pred, the records stitched and cut to R bars; returns the scores (None without)."""
    from style.metrics import NoteMetrics, style_cosines
    from style.sparse import crop_bars, stitch_records
    each = lambda pick: [x for res, live in got for x in pick(res)[:live]]
    bpm = np.asarray(each(lambda res: res.bpm_pred.cpu().tolist()), dtype=np.float64)
    mode = np.asarray(each(lambda res: res.mode_pred.cpu().tolist()), dtype=np.float64).sum(0)
    info = combine_info(style_info=style_info, melody_info=composition_info)
    info['tempo'] = smf.bpm2tempo(round(float(bpm.mean())))
    info['scale'] = dict(info['scale'], mode=major_mode if int(mode.argmax()) == 0 else minor_mode)
    pitched = crop_bars(stitch_records(each(lambda res: res.pitched), bars), R)
    unpitched = crop_bars(stitch_records(each(lambda res: res.unpitched), bars), R) if U else None
    channels_info, unpitched_info = channel_slots(programs)
    mid = decode_records(ChannelConverter(info), channels_info[:C], pitched, unpitched_info if U else None, unpitched)
    mid.save(path)
    if not score:
        return None
    retention = torch.cat([res.retention[:live] for res, live in got]).cpu()
    return dict(cosines=np.concatenate([style_cosines(res.style_sums)[:live] for res, live in got]).mean(0),
                pitched=NoteMetrics(retention[:, :-1]).sum(), unpitched=NoteMetrics(retention[:, -1]).sum())


def get_model_input(path):
    mid = load_midi_from_file(path)
    if mid is None:
        return None
    channels, info = read_midi(mid)
    channels = [c for c in channels if c['instrument_id'] in [-1, *included_instruments]]
    return path, get_input(channels, info)


def extract_style(model, input):
    max_n_bars = 1000 // input[1][1].shape[0]
    mode, bpm, pitched_channels, instruments_features, unpitched_channels = prepare_input(input, max_n_bars)
    with torch.no_grad():
        style, melody, rhythm = model.extract_style(mode, bpm, pitched_channels, instruments_features, unpitched_channels)
    return style.detach(), melody.detach(), rhythm.detach()


def channel_slots(instruments):
    """MIDI channels 0-8, 10-15 for the pitched instruments in order; 9 is percussion (:78-86)."""
    slots = [i for i in range(16) if i != 9]
    pitched = [{'channel_id': slot, 'instrument_id': int(program)} for slot, program in zip(slots, instruments)]
    return pitched, {'channel_id': 9, 'instrument_id': -1}


def save(cc, pitched_channels, unpitched_channels, instruments, save_path, sparse_output=False):
    channels_info, unpitched_info = channel_slots(instruments)
    channels_info = channels_info[:pitched_channels.shape[1]]     # (for numpy rolls shape[1] is the bar count: reference quirk)
    os.makedirs(os.path.dirname(save_path) or '.', exist_ok=True)
    if len(pitched_channels.shape) == 6:                       # numpy rolls straight from get_input
        pitched_channels = torch.tensor(pitched_channels, dtype=torch.float).unsqueeze(0).to(device)
        if unpitched_channels is not None:
            unpitched_channels = torch.tensor(unpitched_channels, dtype=torch.float).unsqueeze(0).to(device)
    mid = decode_midi(cc, channels_info, pitched_channels, unpitched_info, unpitched_channels, sparse_output=sparse_output)
    mid.save(save_path)


def select_instruments(instruments_pred, n_instruments):
    """Top-n of the 41 logits -> (GM programs of the pitched picks, percussion picked?).  A lone
    percussion pick is widened by one so at least one pitched instrument plays (:105-116)."""
    ranked = np.argsort(-np.asarray(instruments_pred))
    picked = ranked[:n_instruments]
    if len(picked) == 1 and picked[0] == percussion_id:
        picked = ranked[:n_instruments + 1]
    unpitched = percussion_id in picked
    programs = [_instrument_categories[i] for i in picked if i != percussion_id]
    return programs, unpitched


def apply_style(model, info, style, melody, rhythm, n_instruments, save_path, sparse_output=False):
    with torch.no_grad():
        instruments_pred, mode, bpm = model.predict_song_info(style, rhythm)
    info['tempo'] = smf.bpm2tempo(round(float(bpm)))
    instruments, unpitched = select_instruments(instruments_pred.detach().cpu().numpy()[0], n_instruments)
    info['scale']['mode'] = major_mode if int(mode[0].argmax()) == 0 else minor_mode
    cc = ChannelConverter(info)
    instruments_features = torch.tensor(encode_instruments(instruments), dtype=torch.float).to(device).unsqueeze(0)
    with torch.no_grad():
        pitched_pred, unpitched_pred = model.apply_style(style, melody, rhythm, instruments_features, unpitched)
    save(cc, pitched_pred, unpitched_pred, instruments, save_path, sparse_output=sparse_output)


def combine_info(style_info, melody_info):
    return {
        'time_signature': melody_info['time_signature'],
        'scale': style_info['scale'],
        'ticks_per_beat': melody_info['ticks_per_beat'],
        'ticks_per_bar': melody_info['ticks_per_bar'],
        'tempo': style_info['tempo'],
    }


def decode_rolls(channel_converter, channels_info, pitched_rolls, unpitched_channel_info=None, unpitched_roll=None):
    """Hard (C,R,T,10,56,5) / (R,T,10,47,2) numpy rolls -> MidiFile; gaps are capped at one second (:145-158)."""
    channels = [channel_converter.vchannel2channel(channel_info, roll)
                for channel_info, roll in zip(channels_info, pitched_rolls)]
    if unpitched_roll is not None:
        channels.append(channel_converter.vchannel2channel(unpitched_channel_info, unpitched_roll))
    return create_midi(channel_converter.info, *channels, max_delta_time=1)


def split_records(pitched_records):
    """Per channel of a pitched SparseRoll of (1, C, R, T, 10, 56, 5): (cells within the channel's roll, feats), in channel order.
    The records are sorted by cell, so the channels are runs of them, cut at multiples of R * T * 10 * 56 cells."""
    n_channels = pitched_records.shape[1]
    per_channel = int(np.prod(pitched_records.shape[2:-1], dtype=np.int64))
    cells, feats = pitched_records.cells.numpy(), pitched_records.feats.numpy()
    cuts = np.searchsorted(cells, per_channel * np.arange(n_channels + 1, dtype=np.int64))
    return [(cells[a:b] - c * per_channel, feats[a:b]) for c, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]


def decode_records(channel_converter, channels_info, pitched_records, unpitched_channel_info=None, unpitched_records=None):
    """`decode_rolls` from the note records of the hard rolls (`style.data.SparseRoll` of (1, C, R, T, 10, 56, 5) /
    (1, 1, R, T, 10, 47, 2)); the channels kept are those `zip(channels_info, pitched_rolls)` keeps."""
    channels = [channel_converter.records2channel(channel_info, pitched_records.shape[2:], cells, feats)
                for channel_info, (cells, feats) in zip(channels_info, split_records(pitched_records))]
    if unpitched_records is not None:
        channels.append(channel_converter.records2channel(unpitched_channel_info, unpitched_records.shape[2:],
                                                          unpitched_records.cells.numpy(), unpitched_records.feats.numpy()))
    return create_midi(channel_converter.info, *channels, max_delta_time=1)


def decode_midi(channel_converter, channels_info, pitched_channels, unpitched_channel_info=None, unpitched_channels=None,
                sparse_output=False):
    if sparse_output:
        pitched_records = hard_output_sparse(pitched_channels)
        unpitched_records = None if unpitched_channels is None else hard_output_sparse(unpitched_channels)
        return decode_records(channel_converter, channels_info, pitched_records, unpitched_channel_info, unpitched_records)
    pitched_rolls = hard_output(pitched_channels).cpu().detach().numpy()[0]
    unpitched_roll = None
    if unpitched_channels is not None:
        unpitched_roll = hard_output(unpitched_channels).cpu().detach().numpy()[0, 0]
    return decode_rolls(channel_converter, channels_info, pitched_rolls, unpitched_channel_info, unpitched_roll)
