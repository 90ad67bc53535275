"""ctypes binding of libmst_amd.so (include/mst_amd.h) — plumbing only.

The product always loads `music-style-transfer_amd/libmst_amd.so` (hipcc, gfx950) and raises
if it is missing: there is no CPU fallback.  Tests may bind another build of the *same* C ABI
(the hipsim interpreter build of the same .hip sources) by passing an explicit path.
"""
import collections
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(os.path.dirname(_HERE), 'libmst_amd.so')

STAGE_EXTRACT, STAGE_INFO, STAGE_APPLY, STAGE_ALL = 1, 2, 4, 7
LOSS_SAVED = 512
LOSS_KEYS = [
    'total', 'channels_loss_total', 'channels_loss_pitched_total', 'channels_loss_pitched_notes_loss',
    'channels_loss_pitched_velocity_loss', 'channels_loss_pitched_duration_loss',
    'channels_loss_pitched_accidentals_loss', 'channels_loss_unpitched_total',
    'channels_loss_unpitched_notes_loss', 'channels_loss_unpitched_velocity_loss',
    'channels_loss_unpitched_duration_loss', 'song_info_loss_total', 'song_info_loss_instruments_loss',
    'song_info_loss_mode_loss', 'song_info_loss_bpm_loss',
]
N_LOSSES = len(LOSS_KEYS)


class MstError(RuntimeError):
    pass


class Dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('C', 'R', 'T', 'beat', 'bar', 'nrf', 'style', 'melody', 'rhythm',
                                         'instr', 'n_instruments', 'has_unpitched', 'clips')]

    def key(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


class PlanOptions(C.Structure):
    _fields_ = [('gemm_tile', C.c_int32), ('no_merge', C.c_int32), ('gemm_run', C.c_int32), ('tile_r0', C.c_int32),
                ('tile_rows', C.c_int32), ('lstm_flavour', C.c_int32), ('dense_flavour', C.c_int32), ('branches', C.c_int32)]


DEV_LSTM_TIMEOUT = 1        # mst_amd.h MST_DEV_LSTM_TIMEOUT
ROLL_NONZERO, ROLL_HARD = 0, 1      # mst_amd.h MST_ROLL_*: record modes of mst_roll_count / mst_roll_compact
WINDOW_WORDS = 4                    # mst_amd.h mst_window: int32 words per descriptor of mst_clip_window (first, count, src_bars, r0)
METRIC_WORDS = 8                    # mst_amd.h MST_METRIC_WORDS: doubles per record of mst_roll_metrics / mst_eval_iteration
ROW_FIELDS = 8                      # mst_amd.h MST_ROW_FIELDS: pieces of a table row one mst_window_inputs call places
STYLE_SUM_WORDS = 8                 # mst_amd.h MST_STYLE_SUM_WORDS: doubles per clip of mst_style_sums
EVAL_ACC_WORDS = 41                 # mst_amd.h MST_EVAL_ACC_WORDS: doubles of a round's running sum (mst_eval_accumulate)
SEARCH_MAX_K = 16                   # mst_amd.h MST_SEARCH_MAX_K: the most neighbours per query of mst_style_search
SEARCH_SLAB = 64                    # mst_amd.h MST_SEARCH_SLAB: rows of the bank one workgroup of mst_style_search owns
ADMIT_DSTS = 16                     # mst_amd.h MST_ADMIT_DSTS: destinations one mst_store_admit call names
SEGMENT_WORDS = 4                   # mst_amd.h mst_segment: int32 words per segment of mst_store_admit (dst, dst_off, src_off, words)


class AdmitDsts:
    """The two destination arrays of mst_store_admit — `ptr[k]` an address (0 = NULL) and `words[k]` its length in 32-bit words —
    made once and passed again with every refresh."""

    def __init__(self, dsts=()):
        self.ptr, self.words = (C.c_void_p * ADMIT_DSTS)(), (C.c_int64 * ADMIT_DSTS)()
        dsts = list(dsts)
        if len(dsts) > ADMIT_DSTS:
            raise MstError(f'mst_store_admit names {ADMIT_DSTS} destinations at most, not {len(dsts)}')
        for k, d in enumerate(dsts):
            self.set(k, *d) if isinstance(d, tuple) else self.set(k, d)

    def set(self, k, t, words=None):
        """Destination k: a 4-byte-element tensor (all of it), or an address and a number of words; None = NULL."""
        if t is None:
            self.ptr[k], self.words[k] = None, 0
        elif isinstance(t, int):
            self.ptr[k], self.words[k] = t or None, int(words)
        else:
            if t.element_size() != 4 or not t.is_contiguous():
                raise MstError('mst_store_admit copies into contiguous tensors of 4-byte elements')
            self.ptr[k], self.words[k] = t.data_ptr(), t.numel() if words is None else int(words)


class RowFields(C.Structure):
    """mst_amd.h mst_row_fields: `n` pieces (src, len) of a table row and the workspace offset `dst` each goes to."""
    _fields_ = [('n', C.c_int32), ('src', C.c_int32 * ROW_FIELDS), ('len', C.c_int32 * ROW_FIELDS), ('dst', C.c_int64 * ROW_FIELDS)]

    @classmethod
    def of(cls, fields):
        """From [(src, len, dst)]."""
        fields = list(fields)
        if not 1 <= len(fields) <= ROW_FIELDS:
            raise MstError(f'mst_row_fields holds 1 to {ROW_FIELDS} fields, not {len(fields)}')
        out = cls(n=len(fields))
        for f, (src, n, dst) in enumerate(fields):
            out.src[f], out.len[f], out.dst[f] = int(src), int(n), int(dst)
        return out


def describe_status(word):
    parts = []
    if word & DEV_LSTM_TIMEOUT:
        parts.append('a granule of the multi-workgroup LSTM exchange did not arrive within 0.2 s (MST_DEV_LSTM_TIMEOUT): the '
                     'launch was not fully resident — something else occupied the GPU next to a batched plan; results since then '
                     'are NaN.  Plan option lstm_flavour=1 (MST_LSTM_FLAVOUR=1) takes the single-workgroup kernels')
    if word & ~DEV_LSTM_TIMEOUT:
        parts.append(f'unknown status bits {word & ~DEV_LSTM_TIMEOUT:#x}')
    return '; '.join(parts)


def options_from_env():
    """Developer switches of the Python binding; the C library itself reads no environment.
    MST_GEMM=mfma|valu forces the 64x64 / 32x32 GEMM tiling, MST_NO_MERGE=1 gives one launch per scheduled member,
    MST_LSTM_FLAVOUR=1 keeps the H = 192 LSTM on one workgroup per sequence (mst_plan_options.lstm_flavour),
    MST_DENSE_FLAVOUR / MST_BRANCHES set mst_plan_options.dense_flavour / .branches."""
    ge = os.environ.get('MST_GEMM')
    if ge not in (None, '', 'mfma', 'valu'):
        raise MstError(f'MST_GEMM={ge!r}: expected mfma or valu')
    return dict(gemm_tile={'mfma': 64, 'valu': 32}.get(ge, 0), no_merge=int(bool(os.environ.get('MST_NO_MERGE'))),
                gemm_run=int(os.environ.get('MST_GEMM_RUN', '0')), lstm_flavour=int(os.environ.get('MST_LSTM_FLAVOUR', '0')),
                dense_flavour=int(os.environ.get('MST_DENSE_FLAVOUR', '0')), branches=int(os.environ.get('MST_BRANCHES', '0')))


_P = C.c_void_p
_SIGS = {
    'mst_param_count': (C.c_int32, [C.POINTER(Dims)]),
    'mst_param_floats': (C.c_int64, [C.POINTER(Dims)]),
    'mst_param_info': (C.c_int32, [C.POINTER(Dims), C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32 * 3)]),
    'mst_widths_supported': (C.c_int32, [C.POINTER(Dims)]),
    'mst_plan_create': (_P, [C.POINTER(Dims), C.POINTER(C.c_int32)]),
    'mst_plan_create_ex': (_P, [C.POINTER(Dims), C.POINTER(PlanOptions), C.POINTER(C.c_int32)]),
    'mst_plan_gemm_tile': (C.c_int32, [_P]),
    'mst_plan_destroy': (None, [_P]),
    'mst_plan_workspace_floats': (C.c_int64, [_P]),
    'mst_plan_tensor': (C.c_int32, [_P, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'mst_plan_launch_count': (C.c_int32, [_P, C.c_int32, C.c_int32]),
    'mst_plan_layout': (C.c_int32, [_P, C.POINTER(C.c_int64 * 4)]),
    'mst_plan_status': (C.c_int32, [_P, _P, C.c_int32, C.POINTER(C.c_int32), _P]),
    'mst_debug_slab_columns_disjoint': (C.c_int32, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    'mst_forward': (C.c_int32, [_P, C.c_int32, _P, _P, _P, _P, _P]),
    'mst_backward': (C.c_int32, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    'mst_zero_grads': (C.c_int32, [_P, C.c_int32, _P, _P]),
    'mst_plan_zero_floats': (C.c_int64, [_P, C.c_int32]),
    'mst_loss_scratch_floats': (C.c_int64, []),
    'mst_total_loss_fwd': (C.c_int32, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, C.c_int32, _P, _P, _P, _P,
                                       C.c_int32, _P, _P, _P, _P]),
    'mst_total_loss_bwd': (C.c_int32, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, C.c_int32, _P, _P, _P, _P,
                                       _P, _P, _P, _P, _P, _P, _P, _P]),
    'mst_train_iteration': (C.c_int32, [_P, _P, _P, _P, _P, _P, _P, _P]),
    'mst_tiled_phase_count': (C.c_int32, [_P]),
    'mst_tiled_phase': (C.c_int32, [_P, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, _P, C.POINTER(C.c_int64 * 8), C.POINTER(C.c_int64 * 8),
                        C.POINTER(C.c_int32)]),
    'mst_adam_step': (C.c_int32, [_P, _P, _P, _P, C.c_int64, _P, C.c_double, C.c_double, C.c_double, C.c_double,
                                  C.c_int32, C.c_double, C.c_int32, _P]),
    'mst_adam_step2': (C.c_int32, [_P, _P, _P, _P, _P, C.c_int64, _P, C.c_double, C.c_double, C.c_double, C.c_double,
                                   C.c_int32, C.c_double, C.c_int32, _P]),
    'mst_grad_guard_scratch_bytes': (C.c_int64, [C.c_int64]),
    'mst_grad_norm': (C.c_int32, [_P, _P, C.c_int64, _P, _P, _P]),
    'mst_grad_norms': (C.c_int32, [_P, _P, _P, _P, C.c_int32, _P, _P]),
    'mst_adam_step_guarded': (C.c_int32, [_P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, _P]),
    'mst_hard_output': (C.c_int32, [_P, _P, C.c_int64, C.c_int32, _P]),
    'mst_clip_scatter': (C.c_int32, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P, _P]),
    'mst_clip_window': (C.c_int32, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _P, _P]),
    'mst_store_admit': (C.c_int32, [_P, C.c_int64, C.c_int32, C.POINTER(C.c_void_p * 16), C.POINTER(C.c_int64 * 16), _P, _P]),
    'mst_roll_slices': (C.c_int64, [C.c_int64]),
    'mst_roll_count': (C.c_int32, [_P, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    'mst_roll_compact': (C.c_int32, [_P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P, _P, _P]),
    'mst_rolls_count': (C.c_int32, [_P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    'mst_rolls_compact': (C.c_int32, [_P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P]),
    'mst_clip_gather': (C.c_int32, [_P, C.c_int32, C.c_int64, _P, C.c_int64, _P, C.c_int32, C.c_int64, _P]),
    'mst_style_sums': (C.c_int32, [_P, C.c_int64, _P, C.c_int32, C.c_int64, _P, C.c_int32, C.c_int64, _P, _P]),
    'mst_style_put': (C.c_int32, [_P, C.c_int64, _P, C.c_int32, C.c_int64, _P, C.c_int32, C.c_int64, _P]),
    'mst_style_mix': (C.c_int32, [_P, C.c_int32, C.c_int64, _P, _P, _P, C.c_int32, _P, C.c_int64, C.c_int32, C.c_int64, _P]),
    'mst_info_decide': (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P,
                                    C.c_int64, _P, _P]),
    'mst_style_search_scratch_bytes': (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    'mst_style_search': (C.c_int32, [_P, C.c_int32, C.c_int64, _P, _P, _P, C.c_int32, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P,
                                     _P, _P]),
    'mst_roll_metrics_scratch_bytes': (C.c_int64, [C.c_int64, C.c_int64]),
    'mst_roll_metrics': (C.c_int32, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P]),
    'mst_eval_scratch_bytes': (C.c_int64, [_P]),
    'mst_eval_iteration': (C.c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'mst_window_inputs': (C.c_int32, [_P, C.c_int32, C.c_int32, _P, C.c_int32, C.POINTER(RowFields), C.c_int64, _P, _P]),
    'mst_eval_accumulate': (C.c_int32, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    'mst_plan_step_count': (C.c_int32, [_P, C.c_int32, C.c_int32]),
    'mst_plan_step_info': (C.c_int32, [_P, C.c_int32, C.c_int32, _P]),
    'mst_plan_step_carried': (C.c_int32, [_P, C.c_int32, C.c_int32, _P]),
    'mst_plan_step_riders': (C.c_int32, [_P, C.c_int32, C.c_int32, _P]),
    'mst_plan_zero_rides': (C.c_int32, [_P]),
    'mst_plan_step_carrier': (C.c_int32, [_P, C.c_int32, C.c_int32, _P]),
    'mst_plan_set_lstm_small': (C.c_int32, [_P, C.c_int32]),
    'mst_plan_step_gemms': (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32]),
    'mst_plan_step_gemm_kinds': (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32]),
    'mst_debug_gemm_walk': (C.c_int64, [C.c_int32] * 11 + [C.POINTER(C.c_int64)]),
    'mst_plan_time_steps': (C.c_int32, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P]),
    'mst_audio_plan_create': (_P, [C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32)]),
    'mst_audio_plan_destroy': (None, [_P]),
    'mst_audio_plan_info': (C.c_int32, [_P, C.POINTER(C.c_int64 * 6)]),
    'mst_audio_stft': (C.c_int32, [_P, _P, _P, _P, _P]),
    'mst_audio_gram': (C.c_int32, [_P, _P, _P, _P, _P]),
    'mst_audio_style_iteration': (C.c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_double, _P]),
    'mst_version': (C.c_char_p, []),
}


def ptr(t):
    """Raw address of a contiguous fp32 tensor (None -> NULL)."""
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise MstError('mst_amd kernels take contiguous float32 tensors')
    return t.data_ptr()


def check(status, what):
    if status != 0:
        names = {-1: 'MST_ERR_ARG', -2: 'MST_ERR_UNSUPPORTED', -3: 'MST_ERR_LAUNCH', -4: 'MST_ERR_ALLOC'}
        raise MstError(f'{what} failed: {names.get(status, status)}')


class Native:
    def __init__(self, path=None):
        path = path or DEFAULT_LIB
        if not os.path.exists(path):
            raise MstError(
                f'{path} not found: the HIP library has not been built. Run `python -c "import __graft_entry__ as g; '
                f'g.build()"` (hipcc --offload-arch=gfx950). There is no CPU fallback.')
        self.path = path
        self.lib = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(self.lib, name)      # raises AttributeError if a declared symbol is missing
            fn.restype, fn.argtypes = res, args
        # plans (schedule + descriptors + a workspace of 100 MB per clip and up) are cached per (dims, device); training on
        # real songs sees a new (C, R) nearly every iteration, so the cache is a small LRU, not a dict that grows forever
        self._plans = collections.OrderedDict()
        self._plan_cap = int(os.environ.get('MST_PLAN_CACHE', '16'))

    # ---- parameter layout
    def param_table(self, dims):
        n = self.lib.mst_param_count(C.byref(dims))
        if n <= 0:
            raise MstError('bad dims')
        out = []
        buf = C.create_string_buffer(256)
        off, nd, shp = C.c_int64(), C.c_int32(), (C.c_int32 * 3)()
        for i in range(n):
            check(self.lib.mst_param_info(C.byref(dims), i, buf, 256, C.byref(off), C.byref(nd), C.byref(shp)), 'mst_param_info')
            out.append((buf.value.decode(), off.value, tuple(shp[k] for k in range(nd.value))))
        return out

    def param_floats(self, dims):
        return self.lib.mst_param_floats(C.byref(dims))

    def clip_scatter(self, cells, feats, counts, out, n_cells, nfeat, n_clips=1, capacity=None, stream=None):
        """mst_clip_scatter: dense `out` (n_clips x n_cells x nfeat floats) from sorted note records.  `cells` (int32), `feats`
        (float32), `counts` (int32) are tensors on out's device or raw addresses; `capacity` = records per clip in the buffers
        (default: cells.numel() // n_clips).  Enqueue-only."""
        if capacity is None:
            capacity = cells.numel() // n_clips
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_clip_scatter(addr(cells), addr(feats), addr(counts), int(capacity), int(n_clips), int(n_cells), int(nfeat),
                                        addr(out), stream), 'mst_clip_scatter')

    def clip_window(self, cells, feats, win, out, n_clips, channels, bars, bar_cells, nfeat, stream=None):
        """mst_clip_window: `out` (n_clips x channels x bars x bar_cells x nfeat floats) cropped out of the songs of a record
        pool.  `cells` (int32) / `feats` (float32) are the pool, `win` the n_clips descriptors (int32 rows of WINDOW_WORDS:
        first, count, src_bars, r0), read on the device.  Tensors on out's device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_clip_window(addr(cells), addr(feats), addr(win), int(n_clips), int(channels), int(bars), int(bar_cells),
                                       int(nfeat), addr(out), stream), 'mst_clip_window')

    def store_admit(self, blob, blob_words, max_segments, dsts, status, stream=None):
        """mst_store_admit: copy the segments a staged `blob` (int32, on the device) lists into the destinations of `dsts` (an
        AdmitDsts), bit for bit; the segment count and the segments are read on the device, `status` (int32, max_segments) says
        per segment 0 = copied or unused, 1 = refused.  Tensors on one device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_store_admit(addr(blob), int(blob_words), int(max_segments), C.byref(dsts.ptr), C.byref(dsts.words),
                                       addr(status), stream), 'mst_store_admit')

    def roll_slices(self, n_cells):
        """mst_roll_slices: slices the compaction kernels cut `n_cells` into; the workspace of roll_count holds one int32 more."""
        n = self.lib.mst_roll_slices(int(n_cells))
        if n <= 0:
            raise MstError(f'mst_roll_slices({n_cells}): need 1 <= n_cells < 2**31')
        return n

    def roll_count(self, x, n_cells, nfeat, mode, ws, stream=None):
        """mst_roll_count: count the records of the dense roll `x` (n_cells x nfeat floats) per slice and scan the counts into
        `ws` (int32, roll_slices(n_cells) + 1): ws[s] = records before slice s, ws[-1] = the total.  `mode`: ROLL_NONZERO or
        ROLL_HARD.  `x`, `ws` are tensors on one device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_roll_count(addr(x), int(n_cells), int(nfeat), int(mode), addr(ws), stream), 'mst_roll_count')

    def roll_compact(self, x, n_cells, nfeat, mode, ws, capacity, cells, feats, stream=None):
        """mst_roll_compact: after roll_count on the same `x`, write the records of rank < `capacity` to `cells` (int32) and
        `feats` (float32, capacity x nfeat) in ascending cell order.  Tensors on x's device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_roll_compact(addr(x), int(n_cells), int(nfeat), int(mode), addr(ws), int(capacity), addr(cells), addr(feats),
                                        stream), 'mst_roll_compact')

    def rolls_count(self, x, roll_stride, n_rolls, n_cells, nfeat, mode, ws, stream=None):
        """mst_rolls_count: roll_count of the `n_rolls` rolls at x + k * roll_stride floats (n_cells x nfeat floats each) into row
        k of `ws` (int32, n_rolls x (roll_slices(n_cells) + 1)).  Tensors on one device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_rolls_count(addr(x), int(roll_stride), int(n_rolls), int(n_cells), int(nfeat), int(mode), addr(ws), stream),
              'mst_rolls_count')

    def rolls_compact(self, x, roll_stride, n_rolls, n_cells, nfeat, mode, ws, capacity, cells, feats, counts, stream=None):
        """mst_rolls_compact: after rolls_count on the same rolls, write the records of rank < `capacity` of roll k to row k of
        `cells` (int32, n_rolls x capacity) and `feats` (float32, n_rolls x capacity x nfeat), and the roll's true number of
        records to counts[k] (int32): mst_clip_scatter's layout.  Tensors on x's device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_rolls_compact(addr(x), int(roll_stride), int(n_rolls), int(n_cells), int(nfeat), int(mode), addr(ws),
                                         int(capacity), addr(cells), addr(feats), addr(counts), stream), 'mst_rolls_compact')

    def clip_gather(self, src, src_rows, src_stride, dst, dst_stride, idx, n_clips, length, stream=None):
        """mst_clip_gather: dst[k * dst_stride + i] = src[idx[k] * src_stride + i] for k < n_clips, i < length, bit for bit.
        `idx` (int32, n_clips) is read on the device, None = identity; an index outside [0, src_rows) gives quiet NaNs.
        Tensors on one device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_clip_gather(addr(src), int(src_rows), int(src_stride), addr(dst), int(dst_stride), addr(idx), int(n_clips),
                                       int(length), stream), 'mst_clip_gather')

    def style_sums(self, a, a_stride, b, b_rows, b_stride, idx, n_clips, length, out, stream=None):
        """mst_style_sums: per clip k the six float64 dot products of x = a + k * a_stride, y = b + idx[k] * b_stride and
        z = b + k * b_stride (`length` floats each) into out[k] (STYLE_SUM_WORDS float64): xx, yy, zz, xy, xz, yz, length, 0.
        `idx` as for clip_gather.  Tensors on one device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_style_sums(addr(a), int(a_stride), addr(b), int(b_rows), int(b_stride), addr(idx), int(n_clips), int(length),
                                      addr(out), stream), 'mst_style_sums')

    def style_put(self, src, src_stride, bank, bank_rows, bank_stride, rows, n_clips, length, stream=None):
        """mst_style_put: bank[rows[k] * bank_stride + i] = src[k * src_stride + i] for k < n_clips, i < length, bit for bit.
        `rows` (int32, n_clips) is read on the device; a row outside [0, bank_rows) writes nothing for that clip.  Tensors on one
        device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_style_put(addr(src), int(src_stride), addr(bank), int(bank_rows), int(bank_stride), addr(rows), int(n_clips),
                                     int(length), stream), 'mst_style_put')

    def style_mix(self, bank, bank_rows, bank_stride, offsets, idx, w, n_entries, dst, dst_stride, n_clips, length, stream=None):
        """mst_style_mix: dst[k * dst_stride + i] = the left-to-right float32 sum over the clip's entries e = offsets[k] ...
        offsets[k + 1] - 1 of w[e] * bank[idx[e] * bank_stride + i], every product and sum rounded on its own.  `offsets` (int32,
        n_clips + 1), `idx` (int32) and `w` (float32, n_entries each) are read on the device; an empty or outlying range or an
        index outside [0, bank_rows) gives quiet NaNs.  Tensors on one device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_style_mix(addr(bank), int(bank_rows), int(bank_stride), addr(offsets), addr(idx), addr(w), int(n_entries),
                                     addr(dst), int(dst_stride), int(n_clips), int(length), stream), 'mst_style_mix')

    def info_decide(self, instruments_pred, mode_pred, bpm_pred, pred_stride, n_logits, group_of, n_groups, channels, n_clips, pool, live,
                    instr, mode, bpm, out_stride, decisions, stream=None):
        """mst_info_decide: per clip the top `channels` pitched instruments of the `n_logits` logits as instrument feature rows
        (`instr`), the one-hot of the larger mode logit (`mode`), rintf(bpm_pred) (`bpm`) and the int32 record of channels + 2
        words (`decisions`: the picks, percussion's rank, the mode index).  `group_of`: a host sequence of n_logits - 1 group
        indices.  `pool`: decide once on the sums over the first `live` clips (one int32 on the device, None = all) and write
        that decision to every clip.  Tensors on one device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        groups = group_of if isinstance(group_of, C.Array) else (C.c_int32 * len(group_of))(*[int(g) for g in group_of])
        check(self.lib.mst_info_decide(addr(instruments_pred), addr(mode_pred), addr(bpm_pred), int(pred_stride), int(n_logits), groups,
                                       int(n_groups), int(channels), int(n_clips), int(bool(pool)), addr(live), addr(instr), addr(mode),
                                       addr(bpm), int(out_stride), addr(decisions), stream), 'mst_info_decide')

    def style_search_scratch_bytes(self, bank_rows, n_queries, k):
        n = self.lib.mst_style_search_scratch_bytes(int(bank_rows), int(n_queries), int(k))
        if n <= 0:
            raise MstError(f'mst_style_search_scratch_bytes: bad arguments ({bank_rows} rows, {n_queries} queries, k = {k})')
        return n

    def style_search(self, bank, bank_rows, bank_stride, n_live, groups, queries, n_queries, query_stride, exclude, length, k, order,
                     rows, scores, scratch, stream=None):
        """mst_style_search: per query the `k` rows of the bank with the largest (order = +1) or smallest (-1) cosine, into
        `rows` (int32, n_queries x k; -1 past the last rankable row) and `scores` (float32, likewise; NaN there).  `n_live` (one
        int32), `groups` (int32 per row) and `exclude` (int32 per query: rows of that group are skipped, -1 skips none) are read
        on the device and may be None.  `scratch`: style_search_scratch_bytes bytes, 8-byte aligned.  Tensors on one device or
        raw addresses.  Two launches, enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_style_search(addr(bank), int(bank_rows), int(bank_stride), addr(n_live), addr(groups), addr(queries),
                                        int(n_queries), int(query_stride), addr(exclude), int(length), int(k), int(order), addr(rows),
                                        addr(scores), addr(scratch), stream), 'mst_style_search')

    def roll_metrics_scratch_bytes(self, n_groups, group_cells):
        n = self.lib.mst_roll_metrics_scratch_bytes(int(n_groups), int(group_cells))
        if n <= 0:
            raise MstError(f'mst_roll_metrics_scratch_bytes({n_groups}, {group_cells}): bad arguments')
        return n

    def roll_metrics(self, pred, target, n_groups, group_cells, nfeat, scratch, out, stream=None):
        """mst_roll_metrics: one record of METRIC_WORDS float64 per group of `group_cells` consecutive cells into `out`, from the
        rolls `pred` and `target` (n_groups x group_cells x nfeat floats each).  `scratch`: roll_metrics_scratch_bytes bytes,
        8-byte aligned.  Tensors on one device or raw addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_roll_metrics(addr(pred), addr(target), int(n_groups), int(group_cells), int(nfeat), addr(scratch), addr(out),
                                        stream), 'mst_roll_metrics')

    def window_inputs(self, table, table_rows, row_floats, rows, n_clips, fields, clip_stride, ws, stream=None):
        """mst_window_inputs: for clip k < n_clips and every field (src, len, dst) of `fields` (a RowFields or a list of such
        triples), ws[dst + k * clip_stride + i] = table[rows[k] * row_floats + src + i], i < len.  `rows` (int32, n_clips) is read
        on the device; a row outside [0, table_rows) gives quiet NaNs.  `table`, `rows`, `ws` are tensors on one device or raw
        addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        if not isinstance(fields, RowFields):
            fields = RowFields.of(fields)
        check(self.lib.mst_window_inputs(addr(table), int(table_rows), int(row_floats), addr(rows), int(n_clips), C.byref(fields),
                                         int(clip_stride), addr(ws), stream), 'mst_window_inputs')

    def eval_accumulate(self, losses, metrics, n_clips, channels, live, acc, stream=None):
        """mst_eval_accumulate: add the first min(max(*live, 0), n_clips) clips of an eval_iteration's `losses` (n_clips x
        N_LOSSES float32) and `metrics` (n_clips x (channels + 2) x METRIC_WORDS float64) into `acc` (EVAL_ACC_WORDS float64), each
        word a left-to-right float64 sum.  `live`: one int32 on the device, or None = all clips.  Tensors on one device or raw
        addresses.  Enqueue-only."""
        addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
        check(self.lib.mst_eval_accumulate(addr(losses), addr(metrics), int(n_clips), int(channels), addr(live), addr(acc), stream),
              'mst_eval_accumulate')

    def plan(self, dims, device):
        opts = options_from_env()
        key = (dims.key(), str(device), tuple(sorted(opts.items())))
        if key in self._plans:
            self._plans.move_to_end(key)
            return self._plans[key]
        plan = self._plans[key] = Plan(self, dims, device, **opts)
        while len(self._plans) > max(1, self._plan_cap):
            self._plans.popitem(last=False)       # the Plan (and its workspace) dies when its last autograd user lets go
        return plan


def current_stream(device):
    if torch.device(device).type == 'cuda':
        return torch.cuda.current_stream(device).cuda_stream
    return None


class Plan:
    """One mst_plan + its workspace tensor. Tensors returned by `view`/`grad` alias the workspace."""
    WS_POOL_CAP = 4

    def __init__(self, native, dims, device, gemm_tile=None, no_merge=None, gemm_run=None, tile_r0=0, tile_rows=0, lstm_flavour=None, dense_flavour=None, branches=None):
        self.native, self.lib, self.dims, self.device = native, native.lib, dims, torch.device(device)
        env = options_from_env()
        opts = PlanOptions(gemm_tile=env['gemm_tile'] if gemm_tile is None else gemm_tile,
                           no_merge=env['no_merge'] if no_merge is None else int(no_merge),
                           gemm_run=env['gemm_run'] if gemm_run is None else int(gemm_run), tile_r0=int(tile_r0), tile_rows=int(tile_rows),
                           lstm_flavour=env['lstm_flavour'] if lstm_flavour is None else int(lstm_flavour),
                           dense_flavour=env['dense_flavour'] if dense_flavour is None else int(dense_flavour),
                           branches=env['branches'] if branches is None else int(branches))
        st = C.c_int32()
        self.handle = self.lib.mst_plan_create_ex(C.byref(dims), C.byref(opts), C.byref(st))
        if not self.handle:
            check(st.value or -1, 'mst_plan_create_ex')
        self.gemm_tile = self.lib.mst_plan_gemm_tile(self.handle)
        self.branches = bool(opts.branches)
        n = self.lib.mst_plan_workspace_floats(self.handle)
        self.ws = torch.zeros(n, dtype=torch.float32, device=self.device)
        self._free_ws = []
        self._touched = {}        # workspaces launched on since the last health check (check_touched)
        self._slots = {}
        lay = (C.c_int64 * 4)()
        check(self.lib.mst_plan_layout(self.handle, C.byref(lay)), 'mst_plan_layout')
        self.clips, self.clip_stride = int(lay[0]), int(lay[1])

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                self.lib.mst_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def slot(self, name):
        if name not in self._slots:
            off, goff, numel = C.c_int64(), C.c_int64(), C.c_int64()
            check(self.lib.mst_plan_tensor(self.handle, name.encode(), C.byref(off), C.byref(goff), C.byref(numel)),
                  f'mst_plan_tensor({name})')
            self._slots[name] = (off.value, goff.value, numel.value)
        return self._slots[name]

    def new_ws(self):
        """A fresh workspace for this plan."""
        return torch.zeros_like(self.ws)

    def acquire_ws(self):
        """A workspace for one grad-enabled forward whose backward is pending: taken from the plan's pool (nothing is
        zero-filled on reuse: every slot is written before it is read), allocated only when the pool is empty.  The pool
        holds FREE workspaces only, so one whose backward never runs is simply garbage-collected."""
        return self._free_ws.pop() if self._free_ws else self.new_ws()

    def release_ws(self, ws):
        if ws is not self.ws and len(self._free_ws) < self.WS_POOL_CAP:
            self._free_ws.append(ws)

    def view(self, name, shape=None, ws=None, clip=0):
        off, _, n = self.slot(name)
        off += clip * self.clip_stride
        t = (self.ws if ws is None else ws)[off:off + n]
        return t.view(*shape) if shape is not None else t

    def grad(self, name, shape=None, ws=None, clip=0):
        _, goff, n = self.slot(name)
        goff += clip * self.clip_stride
        t = (self.ws if ws is None else ws)[goff:goff + n]
        return t.view(*shape) if shape is not None else t

    def set_inputs(self, mode=None, bpm=None, instr=None, used=None, bpm_target=None, ws=None, clip=0):
        for name, t in (('mode', mode), ('bpm', bpm), ('instr', instr), ('used_instruments', used), ('bpm_target', bpm_target)):
            if t is not None:
                self.view(name, ws=ws, clip=clip).copy_(torch.as_tensor(t, dtype=torch.float32).reshape(-1), non_blocking=True)

    def status(self, ws=None, clear=True):
        """Device status word of a workspace (0 = healthy; MST_DEV_* bits otherwise).  Synchronises the current stream."""
        word = C.c_int32()
        check(self.lib.mst_plan_status(self.handle, ptr(self.ws if ws is None else ws), int(bool(clear)), C.byref(word),
                                       current_stream(self.device)), 'mst_plan_status')
        return word.value

    def check_status(self, ws=None):
        word = self.status(ws)
        if word:
            raise MstError('device status: ' + describe_status(word))

    def _touch(self, ws):
        if self.branches and self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            # torch.cuda.graph's capture_end crashes on a capture that forks into this plan's side streams (ROCm 7.2, torch 2.10)
            raise MstError('a plan made with branches=1 cannot run under torch.cuda.graph capture; capture needs branches=0')
        ws = self.ws if ws is None else ws
        self._touched[id(ws)] = ws
        return ws

    def check_touched(self):
        """check_status of every workspace a launch went to since the last call."""
        touched, self._touched = self._touched, {}
        for ws in touched.values():
            self.check_status(ws)

    def launch_count(self, mask=STAGE_ALL, backward=False):
        return self.lib.mst_plan_launch_count(self.handle, mask, int(backward))

    def forward(self, mask, params, pitched, unpitched, ws=None):
        check(self.lib.mst_forward(self.handle, mask, ptr(params), ptr(self._touch(ws)), ptr(pitched),
                                   ptr(unpitched), current_stream(self.device)), 'mst_forward')

    def backward(self, mask, params, gparams, pitched, unpitched, ws=None):
        check(self.lib.mst_backward(self.handle, mask, ptr(params), ptr(gparams), ptr(self._touch(ws)),
                                    ptr(pitched), ptr(unpitched), current_stream(self.device)), 'mst_backward')

    def zero_grads(self, mask, ws=None):
        check(self.lib.mst_zero_grads(self.handle, mask, ptr(self.ws if ws is None else ws), current_stream(self.device)),
              'mst_zero_grads')

    def time_steps(self, mask, backward, params, gparams, pitched, unpitched, reps=20):
        """[(kind, avg_ms, flops, bytes)] per launch step (HIP events on the current stream)."""
        import numpy as np
        n = self.lib.mst_plan_step_count(self.handle, mask, int(backward))
        ms, kind = np.zeros(n, np.float32), np.zeros(n, np.int32)
        fl, by = np.zeros(n, np.float64), np.zeros(n, np.float64)
        got = self.lib.mst_plan_time_steps(self.handle, mask, int(backward), ptr(params), ptr(gparams), ptr(self.ws),
                                           ptr(pitched), ptr(unpitched), current_stream(self.device), reps,
                                           ms.ctypes.data, kind.ctypes.data, fl.ctypes.data, by.ctypes.data)
        if got != n:
            check(got if got < 0 else -1, 'mst_plan_time_steps')
        return list(zip(kind.tolist(), ms.tolist(), fl.tolist(), by.tolist()))

    def step_carried(self, mask=STAGE_ALL, backward=False):
        """One int per step of the pass: 0 = launched on its own, 1 = a gather / segment reduce that its level's GEMM launch
        carries, 2 = carried, with a second stage that is still a launch of its own."""
        import numpy as np
        n = self.lib.mst_plan_step_count(self.handle, mask, int(backward))
        out = np.zeros(n, np.int32)
        got = self.lib.mst_plan_step_carried(self.handle, mask, int(backward), out.ctypes.data)
        check(got if got < 0 else 0, 'mst_plan_step_carried')
        return out.tolist()

    def step_riders(self, mask=STAGE_ALL, backward=False):
        """One int per step of the pass, for every step kind (gathers, segment reduces, combines): 0 = launched on its own,
        1 = the whole step is in its level's GEMM launch, 2 = its first stage is carried and its second stage is a launch
        behind the carrier."""
        import numpy as np
        n = self.lib.mst_plan_step_count(self.handle, mask, int(backward))
        out = np.zeros(n, np.int32)
        got = self.lib.mst_plan_step_riders(self.handle, mask, int(backward), out.ctypes.data)
        check(got if got < 0 else 0, 'mst_plan_step_riders')
        return out.tolist()

    def step_carrier(self, mask=STAGE_ALL, backward=False):
        """One int per step of the pass: the index (in the same list) of the step whose launch runs it, -1 = its own launch."""
        import numpy as np
        n = self.lib.mst_plan_step_count(self.handle, mask, int(backward))
        out = np.zeros(n, np.int32)
        got = self.lib.mst_plan_step_carrier(self.handle, mask, int(backward), out.ctypes.data)
        check(got if got < 0 else 0, 'mst_plan_step_carrier')
        return out.tolist()

    def set_lstm_small(self, on):
        """on = 0: the H <= 16 LSTM launches use the register-flavour kernels instead of the one-wave ones (tests, profiling)."""
        check(self.lib.mst_plan_set_lstm_small(self.handle, int(on)), 'mst_plan_set_lstm_small')

    def zero_rides(self):
        """1 if train_iteration clears the gradient zero list inside its first forward launch, 0 if by a launch of its own."""
        got = self.lib.mst_plan_zero_rides(self.handle)
        check(got if got < 0 else 0, 'mst_plan_zero_rides')
        return got

    def step_gemms(self, mask, backward, step, cap=2048):
        """[(M, N, K, k_splits, fold_rows, workgroups)] of the members (one clip's worth) of GEMM launch step `step`."""
        import numpy as np
        out = np.zeros((cap, 6), np.int32)
        n = self.lib.mst_plan_step_gemms(self.handle, mask, int(backward), step, out.ctypes.data, cap)
        check(n if n < 0 else 0, 'mst_plan_step_gemms')
        return [tuple(r) for r in out[:n].tolist()]

    def step_gemm_kinds(self, mask, backward, step, cap=2048):
        """[(kernel variant, k-tile depth)] of the members of GEMM launch step `step`, in step_gemms' order."""
        import numpy as np
        out = np.zeros((cap, 2), np.int32)
        n = self.lib.mst_plan_step_gemm_kinds(self.handle, mask, int(backward), step, out.ctypes.data, cap)
        check(n if n < 0 else 0, 'mst_plan_step_gemm_kinds')
        return [tuple(r) for r in out[:n].tolist()]

    def tiled_train_iteration(self, params, gparams, pitched, unpitched, losses=None, is_root=True, all_reduce=None):
        """One loop body of a clip whose bars are tiled over ranks (plan made with tile_r0 / tile_rows; `pitched` /
        `unpitched` hold this rank's bars only).  `all_reduce(tensor)` sums a workspace range over the ranks in place —
        torch.distributed.all_reduce by default.  gparams receives this rank's share: all-reduce it before the optimizer step."""
        if all_reduce is None:
            import torch.distributed as dist
            all_reduce = lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM)
        xoff, xlen, nx = (C.c_int64 * 8)(), (C.c_int64 * 8)(), C.c_int32()
        self._touch(None)
        for ph in range(self.lib.mst_tiled_phase_count(self.handle)):
            check(self.lib.mst_tiled_phase(self.handle, ph, ptr(params), ptr(gparams), ptr(self.ws), ptr(pitched), ptr(unpitched),
                                           ptr(losses), int(bool(is_root)), current_stream(self.device), C.byref(xoff), C.byref(xlen),
                                           C.byref(nx)), f'mst_tiled_phase({ph})')
            if nx.value == 1:
                all_reduce(self.ws[xoff[0]:xoff[0] + xlen[0]])
            elif nx.value > 1:
                # the exchanges of one dependency level travel as ONE collective: pack, reduce, unpack
                parts = [self.ws[xoff[q]:xoff[q] + xlen[q]] for q in range(nx.value)]
                total = sum(int(xlen[q]) for q in range(nx.value))
                if getattr(self, '_xstage', None) is None or self._xstage.numel() < total:
                    self._xstage = torch.empty(total, dtype=torch.float32, device=self.device)
                stage = self._xstage[:total]
                torch.cat(parts, out=stage)
                all_reduce(stage)
                at = 0
                for t in parts:
                    t.copy_(stage[at:at + t.numel()])
                    at += t.numel()

    def train_iteration(self, params, gparams, pitched, unpitched, losses=None, ws=None):
        check(self.lib.mst_train_iteration(self.handle, ptr(params), ptr(gparams), ptr(self._touch(ws)),
                                           ptr(pitched), ptr(unpitched), ptr(losses), current_stream(self.device)),
              'mst_train_iteration')

    def eval_scratch(self):
        """The partials buffer of eval_iteration, allocated once per plan."""
        if getattr(self, '_eval_scratch', None) is None:
            n = self.lib.mst_eval_scratch_bytes(self.handle)
            if n <= 0:
                check(int(n) or -1, 'mst_eval_scratch_bytes')
            self._eval_scratch = torch.zeros(n // 8, dtype=torch.float64, device=self.device)
        return self._eval_scratch

    def eval_iteration(self, params, pitched, unpitched, losses, metrics, ws=None):
        """mst_eval_iteration: forward, loss (normalize = 1, the inputs as targets) and note metrics, no backward.  `losses`:
        clips x N_LOSSES float32 (or None), `metrics`: clips x (C + 2) x METRIC_WORDS float64.  Enqueue-only."""
        if metrics.dtype != torch.float64 or not metrics.is_contiguous() or \
                metrics.numel() != self.clips * (self.dims.C + 2) * METRIC_WORDS:
            raise MstError('eval_iteration: metrics must be a contiguous float64 tensor of clips x (C + 2) x 8')
        check(self.lib.mst_eval_iteration(self.handle, ptr(params), ptr(self._touch(ws)), ptr(pitched), ptr(unpitched), ptr(losses),
                                          metrics.data_ptr(), self.eval_scratch().data_ptr(), current_stream(self.device)),
              'mst_eval_iteration')


_native = None


def get():
    """The product library (raises MstError when it has not been built)."""
    global _native
    if _native is None:
        _native = Native()
    return _native
