"""Note metrics of hard_output's decisions: host-side views of the counter records that mst_roll_metrics /
mst_eval_iteration leave on the device (include/mst_amd.h), and the stand-alone `note_metrics` on two GPU rolls.

No reference counterpart: the reference has no validation, and get_total_loss reports soft quantities only.  A record is 8
float64 words; records add, so a sum over channels, clips and songs gives micro-averages.  A ratio with an empty
denominator is NaN, never 0 or 1: "no note predicted" is not a precision."""
import csv
import math
import os

import numpy as np
import torch

from style import _native
from style.utils.misc import assert_dir

WORDS = _native.METRIC_WORDS
NOTE_WORDS = ('cells', 'n_pred', 'n_tgt', 'tp', 'accidentals_ok', 'velocity_abs', 'duration_abs', 'reserved')
SONG_INFO_WORDS = ('n_instruments', 'n_pred', 'n_tgt', 'both', 'mode_ok', 'bpm_abs', 'reserved', 'songs')
NOTE_FIELDS = ('precision', 'recall', 'f1', 'accidentals_accuracy', 'velocity_mae', 'duration_mae')
SONG_INFO_FIELDS = ('instruments_precision', 'instruments_recall', 'instruments_f1', 'mode_accuracy', 'bpm_mae')
VALIDATION_FIELDS = (['iteration', 'clips'] + _native.LOSS_KEYS + [f'pitched_{k}' for k in NOTE_FIELDS] +
                     [f'unpitched_{k}' for k in NOTE_FIELDS if k != 'accidentals_accuracy'] + list(SONG_INFO_FIELDS))


def _ratio(a, b):
    """a / b elementwise with 0 / 0 (and x / 0) = NaN; tensors or numbers."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
        return torch.where(b != 0, a / torch.where(b != 0, b, torch.ones_like(b)), torch.full_like(b, float('nan')))
    return a / b if b != 0 else float('nan')


class _Records:
    """A (..., 8) float64 tensor of counter records, device or host."""
    names = ()

    def __init__(self, words):
        words = torch.as_tensor(words)
        if words.dtype != torch.float64 or words.dim() < 1 or words.shape[-1] != WORDS:
            raise ValueError(f'{type(self).__name__} wraps a (..., {WORDS}) float64 tensor, not {tuple(words.shape)} {words.dtype}')
        self.words = words

    @classmethod
    def zeros(cls, device='cpu'):
        return cls(torch.zeros(WORDS, dtype=torch.float64, device=device))

    def word(self, name):
        return self.words[..., self.names.index(name)]

    def __add__(self, other):
        if type(other) is not type(self):
            return NotImplemented
        return type(self)(self.words + other.words)

    def __radd__(self, other):              # sum([...]) starts from 0
        return self if other == 0 else NotImplemented

    def sum(self):
        """All records of this tensor added into one."""
        return type(self)(self.words.reshape(-1, WORDS).sum(0))

    def cpu(self):
        return type(self)(self.words.cpu())

    def _out(self, x):
        return float(x) if self.words.dim() == 1 else x

    def as_dict(self, prefix=''):
        return {prefix + k: getattr(self, k) for k in self.fields}

    def __repr__(self):
        if self.words.dim() == 1:
            return f'{type(self).__name__}(' + ', '.join(f'{k}={v:.4g}' for k, v in self.as_dict().items()) + ')'
        return f'{type(self).__name__}(shape={tuple(self.words.shape[:-1])})'


class NoteMetrics(_Records):
    """Records of mst_roll_metrics: cells, n_pred (v_pred > .01), n_tgt (v_tgt > 0), TP, TP cells whose hard accidentals equal
    the target's, and the sums over the TP cells of |v_pred - v_tgt| and |d_pred - min(d_tgt, 6)|."""
    names, fields = NOTE_WORDS, NOTE_FIELDS

    @property
    def precision(self):
        return self._out(_ratio(self.word('tp'), self.word('n_pred')))

    @property
    def recall(self):
        return self._out(_ratio(self.word('tp'), self.word('n_tgt')))

    @property
    def f1(self):
        return self._out(_ratio(2 * self.word('tp'), self.word('n_pred') + self.word('n_tgt')))

    @property
    def accidentals_accuracy(self):
        return self._out(_ratio(self.word('accidentals_ok'), self.word('tp')))

    @property
    def velocity_mae(self):
        return self._out(_ratio(self.word('velocity_abs'), self.word('tp')))

    @property
    def duration_mae(self):
        return self._out(_ratio(self.word('duration_abs'), self.word('tp')))


class SongInfoMetrics(_Records):
    """The song-info record of mst_eval_iteration: n_instruments, instruments with logit > 0, with target > .5, with both, mode
    right (0 / 1), |bpm_pred - bpm_target|.  The last word, 0 on the device, counts the songs once `from_device` set it to 1,
    so that sums of records know their denominator."""
    names, fields = SONG_INFO_WORDS, SONG_INFO_FIELDS

    @classmethod
    def from_device(cls, words):
        words = words.clone()
        words[..., 7] = 1.
        return cls(words)

    @property
    def instruments_precision(self):
        return self._out(_ratio(self.word('both'), self.word('n_pred')))

    @property
    def instruments_recall(self):
        return self._out(_ratio(self.word('both'), self.word('n_tgt')))

    @property
    def instruments_f1(self):
        return self._out(_ratio(2 * self.word('both'), self.word('n_pred') + self.word('n_tgt')))

    @property
    def mode_accuracy(self):
        return self._out(_ratio(self.word('mode_ok'), self.word('songs')))

    @property
    def bpm_mae(self):
        return self._out(_ratio(self.word('bpm_abs'), self.word('songs')))


class EvalResult:
    """What StyleTransferModel.eval_iteration returns: `losses` (15 float32 leaves, key order _native.LOSS_KEYS) and `metrics`
    ((C + 2) x 8 float64: the pitched channels, the unpitched roll, the song info), both on the device; nothing is read back
    until a property asks."""

    def __init__(self, losses, metrics):
        self.losses, self.metrics = losses, metrics

    @property
    def pitched(self):
        return NoteMetrics(self.metrics[:-2])

    @property
    def unpitched(self):
        return NoteMetrics(self.metrics[-2])

    @property
    def song_info(self):
        return SongInfoMetrics.from_device(self.metrics[-1])


class TransferResult:
    """What StyleTransferModel.transfer_windows returns for its K clips.  `instruments_pred` (K, 41), `mode_pred` (K, 2) and
    `bpm_pred` (K,) are on the device; `pitched` / `unpitched` are K host SparseRolls each ((1, C, R, T, 10, 56, 5) /
    (1, 1, R, T, 10, 47, 2); `unpitched` is None without percussion): hard_output's note records of the rendered clips.  With
    score=True `style_sums` (K, 8 float64, mst_style_sums' words) and `retention` (K, C + 1, 8 float64, mst_roll_metrics records
    of the written rolls against the clips' own notes: the C pitched channels, then the unpitched roll — zeros without
    percussion) are on the device, else None.  transfer_styles adds `instr_features` (K, C, 51: the instrument rows the clips
    were rendered with) and, where the device decided them, `decisions` (K, C + 2 int32, mst_info_decide's records: the C picked
    logit indices, percussion's position in the ranking, the mode index), both on the device; transfer_windows leaves them None.
    With mix=style.data.Nearest(k) transfer_styles also leaves `neighbours` (K, k int32: the bank rows mst_style_search picked
    for each clip, nearest or farthest first) and `neighbour_scores` (K, k float32: their cosines), on the device; both are None
    for every other mix.  Every tensor is the result's own: a later call does not change it."""

    def __init__(self, instruments_pred, mode_pred, bpm_pred, pitched, unpitched, style_sums=None, retention=None, decisions=None,
                 instr_features=None, neighbours=None, neighbour_scores=None):
        self.instruments_pred, self.mode_pred, self.bpm_pred = instruments_pred, mode_pred, bpm_pred
        self.pitched, self.unpitched, self.style_sums, self.retention = pitched, unpitched, style_sums, retention
        self.decisions, self.instr_features = decisions, instr_features
        self.neighbours, self.neighbour_scores = neighbours, neighbour_scores

    @property
    def cosines(self):
        return style_cosines(self.style_sums)

    @property
    def pitched_retention(self):
        return NoteMetrics(self.retention[:, :-1])

    @property
    def unpitched_retention(self):
        return NoteMetrics(self.retention[:, -1])


def style_cosines(style_sums):
    """mst_style_sums' words (..., 8) -> the three cosines (..., 3) as host float64: the rendered clip's style against the
    donor's (did the style arrive?), against the clip's own (what is left of it), and the clip's own against the donor's — the
    baseline both are read against.  NaN where a norm is 0."""
    s = np.asarray(style_sums.detach().cpu() if torch.is_tensor(style_sums) else style_sums, dtype=np.float64)
    if s.shape[-1] != _native.STYLE_SUM_WORDS:
        raise ValueError(f'style_cosines takes (..., {_native.STYLE_SUM_WORDS}) words, not {s.shape}')
    xx, yy, zz, xy, xz, yz = (s[..., i] for i in range(6))
    with np.errstate(invalid='ignore', divide='ignore'):
        cos = lambda dot, a, b: np.where((a > 0) & (b > 0), dot / (np.sqrt(a) * np.sqrt(b)), np.nan)
        return np.stack([cos(xy, xx, yy), cos(xz, xx, zz), cos(yz, yy, zz)], axis=-1)


def note_metrics(pred, target, per_channel=False):
    """NoteMetrics of two GPU rolls of the model's shapes — (1, C, R, T, 10, 56, 5) or (1, 1, R, T, 10, 47, 2) — as
    get_total_loss is the stand-alone loss.  per_channel=True keeps one record per channel (the roll's second axis), else the
    channels are summed.  The record stays on the device.  There is no CPU fallback."""
    if pred.device.type != 'cuda' or target.device.type != 'cuda':
        raise _native.MstError('note_metrics needs GPU tensors; there is no CPU fallback')
    if pred.shape != target.shape or pred.dim() < 3 or pred.shape[-1] not in (2, 5):
        raise ValueError(f'note_metrics: rolls of shapes {tuple(pred.shape)} / {tuple(target.shape)}')
    dev = pred.device
    pred = pred.detach().to(torch.float32).contiguous()
    target = target.detach().to(dev, torch.float32).contiguous()
    nfeat = pred.shape[-1]
    n_groups = pred.shape[0] * pred.shape[1]
    group_cells = pred.numel() // nfeat // n_groups
    native = _native.get()
    scratch = torch.empty(native.roll_metrics_scratch_bytes(n_groups, group_cells) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(n_groups, WORDS, dtype=torch.float64, device=dev)
    native.roll_metrics(pred, target, n_groups, group_cells, nfeat, scratch, out, _native.current_stream(dev))
    m = NoteMetrics(out)
    return m if per_channel else m.sum()


def validation_row(iteration, clips, losses, pitched, unpitched, song_info):
    """One row of the validation CSV: averaged loss leaves (a NaN leaf — no percussion in any clip — is an empty cell) and the
    derived metrics of the summed records (a 0 / 0 is written as `nan`)."""
    row = dict(iteration=iteration, clips=clips)
    for k, x in zip(_native.LOSS_KEYS, losses):
        row[k] = '' if math.isnan(x) else float(x)
    show = lambda x: 'nan' if math.isnan(x) else x
    row.update({k: show(v) for k, v in pitched.as_dict('pitched_').items()})
    row.update({k: show(v) for k, v in unpitched.as_dict('unpitched_').items() if k != 'unpitched_accidentals_accuracy'})
    row.update({k: show(v) for k, v in song_info.as_dict().items()})
    return row


def append_validation_rows(path, rows):
    """Append rows (validation_row) to the CSV at `path`, fixed columns VALIDATION_FIELDS; the header goes in only when this
    call creates the file, as LossLog does it."""
    assert_dir(path)
    fresh = not os.path.exists(path) or os.path.getsize(path) == 0
    with open(path, 'a', newline='', encoding='utf-8') as f:
        out = csv.writer(f)
        if fresh:
            out.writerow(VALIDATION_FIELDS)
        out.writerows([row[k] for k in VALIDATION_FIELDS] for row in rows)


def round_result(acc):
    """The 41 doubles mst_eval_accumulate summed over a round (include/mst_amd.h), on the host -> the dict
    style.train.evaluate returns: `clips` (acc[0]), `losses` (a leaf is its sum / clips; an unpitched leaf its sum / acc[1], the
    clips with percussion, NaN when there is none — nanmean_leaves' rule), and the three summed records `pitched`, `unpitched`,
    `song_info` (its last word already counts the clips).  `validation_row` applies to it unchanged."""
    acc = np.asarray(torch.as_tensor(acc).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
    if acc.shape != (_native.EVAL_ACC_WORDS,):
        raise ValueError(f'round_result takes the {_native.EVAL_ACC_WORDS} doubles of mst_eval_accumulate, not {acc.shape}')
    n, n_unpitched = acc[0], acc[1]
    sums = acc[2:2 + _native.N_LOSSES]
    losses = sums / n if n else np.full(_native.N_LOSSES, np.nan)
    for i, k in enumerate(_native.LOSS_KEYS):
        if 'unpitched' in k:
            losses[i] = sums[i] / n_unpitched if n_unpitched else np.nan
    records = torch.from_numpy(acc[2 + _native.N_LOSSES:].copy()).reshape(3, WORDS)
    return dict(clips=int(n), losses=losses, pitched=NoteMetrics(records[0]), unpitched=NoteMetrics(records[1]),
                song_info=SongInfoMetrics(records[2]))


def nanmean_leaves(rows):
    """Column means of an (n, 15) array of loss leaves.  The unpitched leaves are NaN for a clip without percussion: they are
    averaged over the clips that have them (NaN when none has).  Any other NaN is a real one and stays."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, _native.N_LOSSES)
    out = rows.mean(0) if len(rows) else np.full(_native.N_LOSSES, np.nan)
    absent = np.isnan(rows[:, _native.LOSS_KEYS.index('channels_loss_unpitched_total')])
    if len(rows) and not absent.all():
        for i, k in enumerate(_native.LOSS_KEYS):
            if 'unpitched' in k:
                out[i] = rows[~absent, i].mean()
    return out
