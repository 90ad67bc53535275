"""The training loop of train-model.py:52-160 as a function, without its per-iteration host syncs.

Same semantics: seed-108 construction order, one song per iteration cut to `800 // C` bars, skipped
empty songs (a skipped iteration also skips the iter_size check), silent percussion dropped, loss with
normalize=True and the positional bpm-before-mode call, gradients accumulated (summed) over
`iter_size` iterations, Adam(lr=.01) + StepLR(200, .9) stepped once per optimizer step, a CSV row and a
progress update per iteration, a whole-module snapshot every `save_interval` iterations.

What is different: the reference reads ~20 scalars back per iteration (`sum() == 0`, `isnan`, `float()`
of every loss leaf).  Here emptiness is decided on the host arrays before upload, the 15 loss leaves of
an iteration stay on the device as one packed tensor, and every `flush_every` iterations ONE copy brings
them back for the CSV rows, the progress bar and the NaN assertion (which therefore fires up to
`flush_every - 1` iterations late).  The optimizer is the fused HIP Adam (style/optim.py).
"""
import csv
import math
import os
import warnings

import numpy as np
import torch

from style import _native
from style.data import (iter_inputs, instrument_size, n_instruments, included_instruments, prepare_input,
                        prepare_input_sparse, get_used_instruments, SongStore)
from style.model import (device, get_total_loss, PitchedChannelsEncoder, UnpitchedChannelsEncoder, PitchedRhythmEncoder,
                         UnpitchedRhythmEncoder, StyleEncoder, MelodyEncoder, SongInfoModel, PitchedStyleApplier,
                         UnpitchedStyleApplier, StyleTransferModel)
from style.metrics import (NoteMetrics, SongInfoMetrics, append_validation_rows, nanmean_leaves, round_result, validation_row,
                           WORDS)
from style.optim import FusedAdam
from style.utils.misc import ProgressBar, assert_dir
from style.utils.parallel import iter_parallel, ParallelIterable

CSV_FIELDS = ['iteration'] + _native.LOSS_KEYS


def build_model(beat_size=64, bar_size=128, n_rhythm_features=8, style_size=256, melody_size=8, rhythm_size=32, seed=108):
    """train-model.py:52-85: same seed, same construction order => same initial weights."""
    torch.manual_seed(seed)
    pce = PitchedChannelsEncoder(beat_size, bar_size, instrument_size).to(device)
    uce = UnpitchedChannelsEncoder(beat_size, bar_size).to(device)
    pre = PitchedRhythmEncoder(rhythm_size, beat_size, bar_size, instrument_size).to(device)
    ure = UnpitchedRhythmEncoder(rhythm_size, beat_size, bar_size).to(device)
    se = StyleEncoder(style_size, bar_size, instrument_size).to(device)
    me = MelodyEncoder(melody_size, beat_size, bar_size, instrument_size).to(device)
    sim = SongInfoModel(n_rhythm_features, style_size, rhythm_size, n_instruments).to(device)
    psa = PitchedStyleApplier(style_size, melody_size, rhythm_size, instrument_size).to(device)
    usa = UnpitchedStyleApplier(style_size, rhythm_size).to(device)
    return StyleTransferModel(pce, uce, se, me, pre, ure, sim, psa, usa)


def drop_silent(input):
    """Host-side version of train-model.py:105-109: None for a song without pitched notes, percussion
    removed when it is silent (within the `800 // C` bars the model will see)."""
    filename, (info, pitched, features, instruments, unpitched) = input
    max_n_bars = 800 // pitched.shape[0]
    if not np.any(pitched[:, :max_n_bars]):
        return None, max_n_bars
    if unpitched is not None and not np.any(unpitched[:, :max_n_bars]):
        unpitched = None
    return (filename, (info, pitched, features, instruments, unpitched)), max_n_bars


def iter_sparse(inputs):
    """The sparse input path's share of the host pipeline, meant for the prefetch thread: every song of `inputs` cut to the
    `800 // C` bars the model will see and turned into note records (style.data.SparseClip) with silence dropped on the
    records as `drop_silent` drops it on the rolls; None stands for a song without pitched notes."""
    for input in inputs:
        max_n_bars = 800 // input[1][1].shape[0]
        # pageable memory: this runs beside the loop thread, which captures hipGraphs, and allocating pinned memory is not
        # allowed while a stream captures; train_iteration stages the records through its own pinned slots
        yield prepare_input_sparse(input, max_n_bars, pin=False).drop_silent()


def fill_store(inputs, n_songs, store=None):
    """The next `n_songs` usable songs of `inputs` (items as `train` takes them) into a style.data.SongStore (a new one on the
    model's device unless given): every song cut to the `800 // C` bars the model would see, songs without pitched notes
    skipped, silent percussion dropped.  Fewer songs go in when `inputs` runs out."""
    store = SongStore(device) if store is None else store
    taken = 0
    while taken < n_songs:
        try:
            input = next(inputs)
        except StopIteration:
            break
        clip = prepare_input_sparse(input, 800 // input[1][1].shape[0], pin=False).drop_silent()
        if clip is None:
            continue
        store.add(clip)
        taken += 1
    return store


class Rotation:
    """The refresh schedule of `train(..., refresh_every=E, refresh_songs=M)`: `songs` yields what iter_sparse yields (a
    SparseClip, or None for a song without pitched notes — skipped), `first_store` builds the ring from the first N usable
    ones and `after(iteration)` admits the next M behind every E-th iteration.  It blocks on `songs`: the schedule is a
    function of their order alone."""

    def __init__(self, songs, every, count):
        self.songs, self.every, self.count = songs, every, count
        self.store, self.too_large, self.exhausted = None, 0, False

    def take(self, n):
        """The next `n` usable songs (fewer when the songs run out) that fit the ring, once there is one."""
        out = []
        while len(out) < n and not self.exhausted:
            try:
                clip = next(self.songs)
            except StopIteration:
                self.exhausted = True
                break
            if clip is None:
                continue
            if self.store is not None and max(clip.pitched_channels.count, 0 if clip.unpitched_channels is None
                                              else clip.unpitched_channels.count) > self.store.capacity:
                self.too_large += 1
                continue
            out.append(clip)
        return out

    def first_store(self, n_songs, records=None):
        if records is not None:                   # (made first: `take` then leaves out the songs that cannot fit)
            self.store = SongStore(device, capacity=int(records), resident=n_songs)
        clips = self.take(n_songs)
        if self.store is None:
            total = max(sum(c.pitched_channels.count for c in clips),
                        sum(c.unpitched_channels.count for c in clips if c.unpitched_channels is not None), 1)
            self.store = SongStore(device, capacity=1 << (2 * total - 1).bit_length(), resident=n_songs)
        self.store.admit(clips)
        return self.store

    def after(self, iteration):
        if (iteration + 1) % self.every == 0 and not self.exhausted:
            clips = self.take(self.count)
            if clips:
                self.store.admit(clips)


class SmallInputStager:
    """The small host inputs of an iteration (mode, bpm, instrument features, used instruments) as ONE asynchronous upload
    through a ring of reusable pinned buffers, so that the loop thread allocates no pinned memory per iteration.  A buffer is
    reused only after the event behind its last copy (long over by then: `slots` iterations have gone by)."""

    def __init__(self, device, slots=4):
        self.device, self.at = device, 0
        self.slots = [dict(buf=None, done=None) for _ in range(slots)]

    def upload(self, *tensors):
        """Device copies of the float32 host tensors (views of one device buffer, on the current stream)."""
        flat = [torch.as_tensor(t, dtype=torch.float32).reshape(-1) for t in tensors]
        n = sum(t.numel() for t in flat)
        slot = self.slots[self.at % len(self.slots)]
        self.at += 1
        if slot['done'] is not None and not slot['done'].query():
            slot['done'].synchronize()
        if slot['buf'] is None or slot['buf'].numel() < n:
            slot['buf'] = torch.empty(max(n, 1 << 12), dtype=torch.float32, pin_memory=True)
        torch.cat(flat, out=slot['buf'][:n])
        dev = slot['buf'][:n].to(self.device, non_blocking=True)
        slot['done'] = slot['done'] or torch.cuda.Event()
        slot['done'].record()
        return tuple(part.view(t.shape) for part, t in zip(dev.split([t.numel() for t in flat]), tensors))


class LossLog:
    """Packed loss tensors of the iterations since the last flush."""

    def __init__(self, path, pbar, flush_every, health=None, tolerate_nan=False, guard_stats=None):
        self.path, self.pbar, self.flush_every = path, pbar, flush_every
        self.health = health          # callable raising on a device-side failure (StyleTransferModel.check_device_status)
        self.tolerate_nan = tolerate_nan      # a NaN loss is written as a row (the optimizer skips such a step) instead of asserted on
        self.guard_stats = guard_stats        # callable returning FusedAdam.guard_stats() (or None): shown by the progress meter
        self.pending = []

    def add(self, iteration, packed):
        self.pending.append((iteration, packed))
        if len(self.pending) >= self.flush_every:
            self.flush()

    def flush(self):
        if not self.pending:
            return
        if self.health is not None:
            self.health()             # joins the model's accumulation lanes; a kernel-reported failure names itself here
        values = torch.stack([p for _, p in self.pending]).cpu().numpy()          # the one D2H copy
        rows = []
        for (iteration, _), v in zip(self.pending, values):
            leaf = dict(zip(_native.LOSS_KEYS, v.tolist()))
            assert self.tolerate_nan or not math.isnan(leaf['total']), f'loss is NaN at iteration {iteration}'
            has_u = not math.isnan(leaf['channels_loss_unpitched_total'])
            row = dict(iteration=iteration, **{k: ('' if math.isnan(x) else x) for k, x in leaf.items()})
            if math.isnan(leaf['total']):
                row['total'] = 'nan'          # tolerated: the row says so, where an absent leaf is an empty cell
            rows.append(row)
            if self.pbar is not None and math.isnan(leaf['total']):
                self.pbar.add(1)              # counted, but kept out of the meter's averages
            elif self.pbar is not None:
                self.pbar.add(1, total_loss=leaf['total'], pitched_loss=leaf['channels_loss_pitched_total'],
                              pitched_notes_loss=leaf['channels_loss_pitched_notes_loss'],
                              song_info_loss=leaf['song_info_loss_total'],
                              instruments_loss=leaf['song_info_loss_instruments_loss'],
                              channelss_loss=leaf['channels_loss_total'], mode_loss=leaf['song_info_loss_mode_loss'],
                              bpm_loss=leaf['song_info_loss_bpm_loss'])
                if has_u:
                    self.pbar.update_values(1, unpitched_loss=leaf['channels_loss_unpitched_total'],
                                            unpitched_notes_loss=leaf['channels_loss_unpitched_notes_loss'])
        stats = self.guard_stats() if self.guard_stats is not None and self.pbar is not None else None
        if stats is not None:
            # at the flush, where the loop synchronises anyway; the CSV keeps its columns.  Shown as they are (the last step's
            # norm, the count of skipped steps), not momentum-averaged: their running sums start afresh
            for k in ('grad_norm', 'skipped'):
                self.pbar.values_sum.pop(k, None)
                self.pbar.values_seen.pop(k, None)
            self.pbar.update_values(1, grad_norm=stats['norm'] if math.isfinite(stats['norm']) else None,
                                    skipped=float(stats['steps_skipped']))
        if self.path:
            self._append_rows(rows)
        self.pending = []

    def _append_rows(self, rows):
        """One CSV row per iteration with the flattened loss leaves (train-model.py:148-149), fixed columns
        CSV_FIELDS; the header goes in only when this call creates the file."""
        assert_dir(self.path)
        fresh = not os.path.exists(self.path) or os.path.getsize(self.path) == 0
        with open(self.path, 'a', newline='', encoding='utf-8') as f:
            out = csv.writer(f)
            if fresh:
                out.writerow(CSV_FIELDS)
            out.writerows([row[k] for k in CSV_FIELDS] for row in rows)


def evaluate(model, inputs, n_clips, sparse_input=False):
    """One held-out evaluation round: the next `n_clips` songs of `inputs` (items as `train` takes them) through
    StyleTransferModel.eval_iteration — forward, loss and note metrics, no backward, no gradient, no optimizer.  The songs
    are cut to `800 // C` bars and silence is treated as in the training loop: a song without pitched notes is skipped, not
    counted; silent percussion is dropped.  sparse_input=True uploads the note tensors as note records.  Everything stays on
    the device until ONE copy at the end.  Returns dict(clips, losses, pitched, unpitched, song_info): the loss leaves averaged
    over the clips (a numpy array in style._native.LOSS_KEYS order; the unpitched leaves over the clips with percussion) and
    the records summed over channels and clips (style.metrics.NoteMetrics / SongInfoMetrics, on the host), i.e.
    micro-averages.  Fewer than `n_clips` clips are evaluated when `inputs` runs out."""
    rows = []
    while len(rows) < n_clips:
        try:
            input = next(inputs)
        except StopIteration:
            break
        if sparse_input:
            clip = prepare_input_sparse(input, 800 // input[1][1].shape[0]).drop_silent()
            if clip is None:
                continue
            mode, bpm, pitched, features, unpitched = clip
            bpm_target = clip.bpm_target
        else:
            input, max_n_bars = drop_silent(input)
            if input is None:
                continue
            mode, bpm, pitched, features, unpitched = prepare_input(input, max_n_bars)
            bpm_target = input[1][0]['bpm']
        used = get_used_instruments(features, unpitched)
        res = model.eval_iteration(mode, bpm, pitched, features, unpitched, used, bpm_target)
        # a song's (C + 2) records as three: the pitched channels summed, the unpitched roll, the song info
        rows.append(torch.cat([res.losses.double(), res.metrics[:-2].sum(0), res.metrics[-2], res.metrics[-1]]))
    n = len(rows)
    host = torch.stack(rows).cpu() if n else torch.zeros(0, _native.N_LOSSES + 3 * WORDS, dtype=torch.float64)     # the one D2H copy
    records = host[:, _native.N_LOSSES:].reshape(n, 3, WORDS)
    return dict(clips=n, losses=nanmean_leaves(host[:, :_native.N_LOSSES].numpy()), pitched=NoteMetrics(records[:, 0]).sum(),
                unpitched=NoteMetrics(records[:, 1]).sum(), song_info=SongInfoMetrics.from_device(records[:, 2]).sum())


def evaluate_windows(model, store, bars, K, stride=None):
    """One held-out round over the store's fixed set of windows (style.data.SongStore.window_batches(bars, K, stride)): every
    batch, across shape buckets, goes through StyleTransferModel.eval_windows into ONE accumulator the model owns (zeroed
    here; records add, and the pitched record is already summed over the channels, so buckets of different C share it) — per
    batch one small upload and one graph replay, at the end ONE copy of 41 doubles to the host.  The padding of a bucket's
    last batch is not scored.  Every round scores the same windows, so rounds are comparable.  Returns `evaluate`'s dict
    (style.metrics.round_result: clips = the windows counted) plus `windows_skipped`, the windows the silence rule left out."""
    batches = store.window_batches(bars, K, stride)
    acc = model.eval_accumulator()
    acc.zero_()
    for batch, live in batches:
        model.eval_windows(store, batch, live=live, acc=acc)
    result = round_result(acc.cpu())                  # the one D2H copy
    result['windows_skipped'] = batches.skipped
    return result


def train(model, inputs, n_iterations=5000, iter_size=2, training_info_path='training.csv', save_path='snapshots/',
          save_interval=100, flush_every=20, progress=True, optimizer=None, fused=True, sparse_input=False,
          max_grad_norm=None, skip_nonfinite=False, save_optimizer=False, eval_inputs=None, eval_every=0, eval_clips=8,
          eval_info_path='validation.csv', batch_clips=None, window_bars=16, store_songs=64, window_seed=0, eval_windows=None,
          refresh_every=None, refresh_songs=4, store_records=None):
    """`inputs`: iterator of (filename, get_input(...)) tuples, e.g. iter_parallel(iter_inputs(...)).
    fused=True runs a loop body as ONE C-ABI call (StyleTransferModel.train_iteration: same arithmetic, same gradients, no
    autograd graph); fused=False is the reference's own sequence model(...) -> get_total_loss -> backward.
    sparse_input=True feeds the note tensors as sorted note records: a prefetch thread cuts and sparsifies the songs
    (iter_sparse), this loop only enqueues the upload of the records (a few hundred KB at most, through pinned memory) and the
    kernel that builds the dense tensors on the device (mst_clip_scatter).  Same tensors bit for bit, hence the same losses.
    The prefetch thread runs ahead of the loop: when train() returns it has taken one or two songs more from `inputs` than
    the loop used, and it is told to stop and joined for up to 5 s — a daemon thread that is still blocked inside the
    caller's iterator after that (a slow parse) ends with it.
    max_grad_norm / skip_nonfinite configure the default FusedAdam's guard (global gradient-norm clipping, and skipping a step
    whose gradient norm is inf / NaN — decided on the device, inside the optimizer step); with an `optimizer` of the caller's
    they are refused: configure that optimizer instead.  With skip_nonfinite a NaN loss is logged as a row, not asserted on.
    save_optimizer=True writes optimizer.state_dict() as `{iteration}.optim.pkl` beside every model snapshot.
    eval_inputs (an iterator of held-out songs, items as `inputs`) with eval_every = N > 0 runs one `evaluate` round of
    `eval_clips` songs after every N-th iteration and appends a row to `eval_info_path` (style.metrics.VALIDATION_FIELDS: the
    iteration, the clip count, the averaged loss leaves and the note / song-info metrics of hard_output's decisions); the
    progress meter shows `val_f1`.  Evaluation forms no gradient and leaves the training bits alone; with eval_inputs=None the
    loop is what it is without this argument.
    batch_clips = K switches to windowed batches: before the loop the next `store_songs` usable songs of `inputs` (cut to
    `800 // C` bars as always; songs without pitched notes are skipped, silent percussion is dropped) go into a
    style.data.SongStore on the device, and every iteration is then `store.sample(rng, K, window_bars)` — K windows of
    `window_bars` bars of songs of one shape bucket, drawn by numpy.random.default_rng(window_seed) —
    StyleTransferModel.train_windows (one batched pass over the K windows, cropped on the device) and optimizer.step().  One
    CSV row per iteration holds the loss leaves averaged over the K clips (on the device).  `iter_size` is ignored with a
    warning: K takes its place.  Needs fused=True; sparse_input only decides how evaluation rounds upload their songs.
    batch_clips=None leaves the loop exactly as it is.
    eval_windows = M (with batch_clips and eval_inputs; ValueError otherwise) makes validation follow: before the loop the next M
    usable songs of `eval_inputs` go into a second SongStore, and every due round is `evaluate_windows` over that store's fixed
    windows of `window_bars` bars in batches of `batch_clips` — the same windows every round, summed on the device.  `eval_clips`
    is not used then; the CSV's `clips` column is the number of windows counted.  eval_windows=None: every path is as above.
    refresh_every = E (with batch_clips; ValueError otherwise) rotates the songs through a fixed ring on the device, so that the
    batched loop trains on all of `inputs` in fixed device memory: the first `store_songs` = N usable songs are sparsified on
    the host and admitted as one group to a SongStore(resident=N) whose pools hold `store_records` records each (default: twice
    the larger pool's records of those N songs, rounded up to a power of two); after every E-th iteration — (iteration + 1) % E
    == 0, behind optimizer.step() — the next `refresh_songs` = M usable songs are admitted (SongStore.admit: one upload, one
    mst_store_admit launch) and the oldest leave.  No address moves, so train_windows' captured graph keeps replaying.  The
    songs come from a prefetch thread (iter_sparse, as for sparse_input, stopped and joined the same way) and the loop WAITS
    for its M songs: which songs are resident at which iteration depends on the order of `inputs` alone, never on timing.  A
    song too large for the ring is skipped and counted (a warning at the end says how many); when `inputs` runs out, what it
    still gave is admitted, refreshing stops and training goes on.  The ring's status words are read where the loop
    synchronises anyway (the flush).  refresh_every=None: the loop, the append-only store included, is what it is without
    this argument."""
    if optimizer is not None and (max_grad_norm is not None or skip_nonfinite):
        raise ValueError('max_grad_norm / skip_nonfinite configure the default optimizer; with optimizer= set them on that optimizer')
    if eval_windows is not None and (batch_clips is None or eval_inputs is None or int(eval_windows) < 1):
        raise ValueError('eval_windows = M >= 1 needs batch_clips (the shape and batch size of the windows) and eval_inputs (the '
                         'held-out songs)')
    if refresh_every is not None and (batch_clips is None or int(refresh_every) < 1 or int(refresh_songs) < 1 or
                                      (store_records is not None and int(store_records) < 1)):
        raise ValueError('refresh_every = E >= 1 needs batch_clips (the rotating store feeds windowed batches), refresh_songs >= 1 '
                         'and, when given, store_records >= 1')
    windows, feeder, rotation = None, None, None
    if batch_clips is not None:
        if not fused:
            raise ValueError('batch_clips needs fused=True: windowed batches run through StyleTransferModel.train_windows')
        if int(batch_clips) < 1 or int(window_bars) < 1 or int(store_songs) < 1:
            raise ValueError('batch_clips, window_bars and store_songs must be at least 1')
        if iter_size != 1:
            warnings.warn(f'iter_size={iter_size} is ignored with batch_clips: the optimizer steps after every batch of {batch_clips} clips')
        if refresh_every is None:
            store = fill_store(inputs, int(store_songs))
        else:
            feeder = ParallelIterable(iter_sparse(inputs))
            try:
                rotation = Rotation(iter(feeder), int(refresh_every), int(refresh_songs))
                store = rotation.first_store(int(store_songs), store_records)
            except BaseException:
                feeder.stop(timeout=5.)
                raise
        windows = (store, np.random.default_rng(window_seed), int(batch_clips), int(window_bars))
    if sparse_input and windows is None:
        feeder = ParallelIterable(iter_sparse(inputs))
        inputs = iter(feeder)
    try:
        if windows is not None and not len(windows[0]):
            raise ValueError('batch_clips: `inputs` held no usable song')
        eval_store = None
        if eval_windows is not None:
            eval_store = fill_store(eval_inputs, int(eval_windows))
            if not len(eval_store):
                raise ValueError('eval_windows: `eval_inputs` held no usable song')
        return _train_loop(model, inputs, n_iterations, iter_size, training_info_path, save_path, save_interval, flush_every,
                           progress, optimizer, fused, sparse_input, max_grad_norm, skip_nonfinite, save_optimizer,
                           eval_inputs if eval_every and eval_every > 0 else None, eval_every, eval_clips, eval_info_path, windows,
                           eval_store, rotation)
    finally:
        if feeder is not None:
            feeder.stop(timeout=5.)
        if rotation is not None and rotation.too_large:
            warnings.warn(f'refresh_every: {rotation.too_large} songs hold more records than the ring (store_records) and were skipped')


def _train_loop(model, inputs, n_iterations, iter_size, training_info_path, save_path, save_interval, flush_every, progress,
                optimizer, fused, sparse_input, max_grad_norm=None, skip_nonfinite=False, save_optimizer=False,
                eval_inputs=None, eval_every=0, eval_clips=8, eval_info_path='validation.csv', windows=None, eval_store=None,
                rotation=None):
    optimizer = optimizer or FusedAdam(model, lr=.01, step_size=200, gamma=.9, max_grad_norm=max_grad_norm,
                                       skip_nonfinite=skip_nonfinite)
    optimizer.zero_grad()
    pbar = ProgressBar(n_iterations) if progress else None
    health = getattr(model, 'check_device_status', None)
    if rotation is not None:
        model_health = health

        def health():                     # at the flush, where the loop synchronises anyway
            if model_health is not None:
                model_health()
            rotation.store.check()
    log = LossLog(training_info_path, pbar, flush_every, health=health,
                  tolerate_nan=bool(getattr(optimizer, 'skip_nonfinite', False)), guard_stats=getattr(optimizer, 'guard_stats', None))
    stager = SmallInputStager(device) if sparse_input and windows is None else None
    for iteration in range(n_iterations):
        if windows is not None:
            store, rng, batch_clips, window_bars = windows
            batch = store.sample(rng, batch_clips, window_bars)
            if batch is None:
                raise ValueError(f'no bucket of the store holds a song with a sounding window of {window_bars} bars')
            packed = model.train_windows(store, batch).mean(0)      # one row per iteration: the leaves averaged over the K clips
            log.add(iteration, packed)
            optimizer.step()                      # K clips have accumulated: K takes iter_size's place
            if rotation is not None:
                rotation.after(iteration)
            _after_iteration(model, optimizer, log, pbar, iteration, eval_inputs, eval_every, eval_clips, eval_info_path,
                             sparse_input, save_interval, save_path, save_optimizer,
                             None if eval_store is None else (eval_store, window_bars, batch_clips))
            continue
        if sparse_input:
            input = next(inputs)
        else:
            input, max_n_bars = drop_silent(next(inputs))
        if input is None:
            if pbar is not None:
                pbar.n_iterations -= 1
            continue
        if sparse_input:
            info = dict(bpm=input.bpm_target)
            mode, bpm, pitched, features, unpitched = input
            mode, bpm, features, used = stager.upload(mode, bpm, features, get_used_instruments(features, unpitched))
            if not fused:                          # the autograd path's loss reads the dense targets
                pitched, unpitched = model._dense(pitched), model._dense(unpitched)
        else:
            info = input[1][0]
            mode, bpm, pitched, features, unpitched = prepare_input(input, max_n_bars)
            used = get_used_instruments(features, unpitched)
        if fused:
            packed = model.train_iteration(mode, bpm, pitched, features, unpitched, used, info['bpm'])
        else:
            (instruments_pred, mode_pred, bpm_pred), pitched_pred, unpitched_pred = model(mode, bpm, pitched, features, unpitched)
            losses = get_total_loss(instruments_pred, used, bpm_pred, info['bpm'], mode_pred, mode, pitched_pred, pitched,
                                    unpitched_pred, unpitched, normalize=True)
            losses['total'].backward()
            packed = losses.packed
        log.add(iteration, packed)
        if (iteration + 1) % iter_size == 0:
            optimizer.step()                      # Adam + StepLR + zero_grad in one launch
        _after_iteration(model, optimizer, log, pbar, iteration, eval_inputs, eval_every, eval_clips, eval_info_path, sparse_input,
                         save_interval, save_path, save_optimizer)
    log.flush()
    return model


def _after_iteration(model, optimizer, log, pbar, iteration, eval_inputs, eval_every, eval_clips, eval_info_path, sparse_input,
                     save_interval, save_path, save_optimizer, eval_windowed=None):
    """What follows the optimizer step of an iteration: the evaluation round and the snapshot that are due.  `eval_windowed`:
    (store, bars, K) of a windowed round (evaluate_windows) in place of `evaluate`."""
    if eval_inputs is not None and (iteration + 1) % eval_every == 0:
        if eval_windowed is not None:
            result = evaluate_windows(model, *eval_windowed)
        else:
            result = evaluate(model, eval_inputs, eval_clips, sparse_input=sparse_input)
        if eval_info_path:
            append_validation_rows(eval_info_path, [validation_row(iteration, result['clips'], result['losses'], result['pitched'],
                                                                   result['unpitched'], result['song_info'])])
        if pbar is not None and not math.isnan(result['pitched'].f1):
            for k in (pbar.values_sum, pbar.values_seen):       # shown as it is (the last round's), not momentum-averaged
                k.pop('val_f1', None)
            pbar.update_values(1, val_f1=result['pitched'].f1)
    if iteration % save_interval == 0 and save_path:
        log.flush()
        path = os.path.join(save_path, f'{iteration}.pkl')
        assert_dir(path)
        with open(path, 'wb') as f:
            torch.save(model, f)
        if save_optimizer:
            with open(os.path.join(save_path, f'{iteration}.optim.pkl'), 'wb') as f:
                torch.save(optimizer.state_dict(), f)


def split_eval_files(files, n_eval_files):
    """(training files, held-out files): the files sorted, the last `n_eval_files` of them held out."""
    files = sorted(files)
    n = max(0, min(int(n_eval_files), len(files)))
    return files[:len(files) - n], files[len(files) - n:]


def main(data_path='data/Lakh MIDI Dataset/clean_midi/', n_eval_files=0, **kwargs):
    """n_eval_files > 0 holds the last that many of the sorted files out of the training list and cycles them as the
    `eval_inputs` of `train` (give eval_every as well)."""
    from style.utils.misc import iter_all_files
    print(f'Using {device}')
    print('Listing data files')
    files = list(iter_all_files(data_path, '**/*.mid'))
    held_out = []
    if n_eval_files:
        files, held_out = split_eval_files(files, n_eval_files)
    print('Creating model')
    model = build_model()
    print('Training')
    inputs = iter_parallel(iter_inputs(files, included_instruments, shuffle=True, looped=True))
    if held_out:
        kwargs['eval_inputs'] = iter_parallel(iter_inputs(held_out, included_instruments, shuffle=False, looped=True))
    return train(model, inputs, **kwargs)
