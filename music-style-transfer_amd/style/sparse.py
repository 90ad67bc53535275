"""Piano rolls as sorted note records (`style.data.SparseRoll`, re-exported there).

A roll is > 98 % zeros: a song holds 400 to 6100 non-zero cells in 2 to 37 MB of float32.  A SparseRoll keeps, per non-zero
cell, its flat index (C order of the roll without the feature axis) and its 5 / 2 features.  The host keeps them in ONE int32
buffer — header, cells, feature bits — so a clip goes to the device as one copy of a few hundred KB at most, and
mst_clip_scatter builds the dense tensor the kernels read there.  `densify(sparsify(x))` is `x.astype(float32)` bit for bit.

No reference counterpart: the reference uploads dense rolls (style/data.py:130-156).
"""
import numpy as np
import torch

from style import _native

HEADER = 4            # int32 words in front of the cells: [count, 0, 0, 0] (keeps the cells 16-byte aligned)


def _cells_words(count):
    """Words the cells take in the packed buffer: padded to a multiple of 4 (so the features stay 16-byte aligned), never 0."""
    return max(4, (count + 3) & ~3)


def packed_words(count, nfeat):
    return HEADER + _cells_words(count) + count * nfeat


class SparseRoll:
    """Note records of one dense roll of `shape` (feature axis last): `cells` int32 (n,), strictly ascending; `feats` float32
    (n, nfeat).  Both are views of `packed`, the int32 buffer that is uploaded; `pin=True` puts it in pinned host memory
    (default: when a GPU is present)."""

    def __init__(self, cells, feats, shape, pin=None):
        shape, nfeat, n_cells = self._geometry(shape)
        cells = np.ascontiguousarray(torch.as_tensor(cells).numpy() if torch.is_tensor(cells) else cells)
        feats = np.ascontiguousarray(torch.as_tensor(feats).numpy() if torch.is_tensor(feats) else feats)
        if cells.ndim != 1 or cells.dtype.kind not in 'iu':
            raise ValueError('cells: a 1-d integer array')
        n = cells.shape[0]
        feats = feats.reshape(n, nfeat) if feats.size == n * nfeat else feats
        if feats.shape != (n, nfeat):
            raise ValueError(f'feats: shape {feats.shape}, expected {(n, nfeat)}')
        self._check_cells(cells, n_cells)
        if pin is None:
            pin = torch.cuda.is_available()
        self._adopt(torch.zeros(packed_words(n, nfeat), dtype=torch.int32, pin_memory=bool(pin)), n, shape, nfeat, n_cells)
        self.packed[0] = n
        self.cells.numpy()[:] = cells
        self.feats.numpy()[:] = feats.astype(np.float32, copy=False)

    @staticmethod
    def _geometry(shape):
        shape = tuple(int(d) for d in shape)
        if len(shape) < 2 or shape[-1] not in (2, 5):
            raise ValueError(f'shape {shape}: the last axis holds the 5 pitched or 2 unpitched note features')
        n_cells = int(np.prod(shape[:-1], dtype=np.int64))
        if not 1 <= n_cells < 2 ** 31:
            raise ValueError(f'shape {shape}: {n_cells} cells, need 1 <= cells < 2**31')
        return shape, shape[-1], n_cells

    @staticmethod
    def _check_cells(cells, n_cells):
        if len(cells):
            c64 = cells.astype(np.int64)
            if c64.min() < 0 or c64.max() >= n_cells:
                raise ValueError(f'cells out of range [0, {n_cells})')
            if np.any(np.diff(c64) <= 0):
                raise ValueError('cells must be strictly ascending (sorted, no duplicates)')

    def _adopt(self, packed, n, shape, nfeat, n_cells):
        self.shape, self.nfeat, self.n_cells, self.count = shape, nfeat, n_cells, n
        self.packed = packed
        at = HEADER + _cells_words(n)
        self.cells = packed[HEADER:HEADER + n]
        self.feats = packed[at:at + n * nfeat].view(torch.float32).view(n, nfeat)

    @classmethod
    def from_packed(cls, packed, shape):
        """Adopt `packed` — a contiguous host int32 tensor in the packed layout, its header word holding the count — as the
        records of a roll of `shape`: no copy, `cells` / `feats` are views of it.  The same validation as the constructor."""
        shape, nfeat, n_cells = cls._geometry(shape)
        if not torch.is_tensor(packed) or packed.dtype != torch.int32 or packed.dim() != 1 or packed.device.type != 'cpu' or \
                not packed.is_contiguous() or packed.numel() < HEADER:
            raise ValueError('packed: a contiguous 1-d int32 host tensor with the 4-word header')
        n = int(packed[0])
        if n < 0 or packed.numel() != packed_words(n, nfeat):
            raise ValueError(f'packed: {packed.numel()} words do not hold {n} records of {nfeat} features')
        roll = cls.__new__(cls)
        roll._adopt(packed, n, shape, nfeat, n_cells)
        cls._check_cells(roll.cells.numpy(), n_cells)
        return roll

    def __repr__(self):
        return f'SparseRoll(shape={self.shape}, records={self.count})'

    def any(self):
        """np.any of the dense roll, from the records."""
        return bool(np.any(self.feats.numpy()))

    def to_numpy(self):
        """The dense float32 roll, built on the host."""
        out = np.zeros((self.n_cells, self.nfeat), dtype=np.float32)
        out[self.cells.numpy()] = self.feats.numpy()
        return out.reshape(self.shape)

    def to_dense(self, device, out=None, native=None):
        """The dense float32 roll on `device`, built there by mst_clip_scatter on the current stream (the records are uploaded
        asynchronously when they are pinned).  `out`: a contiguous float32 tensor of the roll's size to write into — every float
        of it is overwritten.  `native`: another build of the C ABI (tests: the CPU interpreter build)."""
        device = torch.device(device)
        if out is None:
            out = torch.empty(self.shape, dtype=torch.float32, device=device)
        elif out.numel() != self.n_cells * self.nfeat or out.dtype != torch.float32 or not out.is_contiguous():
            raise _native.MstError('to_dense(out=): a contiguous float32 tensor with the roll\'s number of elements')
        records = self.packed.to(device, non_blocking=True) if device.type == 'cuda' else self.packed
        scatter_packed(native or _native.get(), records, self.count, self.n_cells, self.nfeat, out, _native.current_stream(device))
        return out


def scatter_packed(native, records, count, n_cells, nfeat, out, stream):
    """Enqueue mst_clip_scatter over a packed record buffer (SparseRoll.packed, or its copy on out's device)."""
    base = records.data_ptr()
    cells = base + 4 * HEADER
    native.clip_scatter(cells, cells + 4 * _cells_words(count), base, out, n_cells, nfeat, n_clips=1, capacity=count, stream=stream)


def sparsify(roll, pin=None):
    """Dense roll (any float dtype, feature axis last) -> SparseRoll.  The roll is converted to float32 FIRST; a cell is kept
    when the float32 bit pattern of any of its features is not all-zero (so -0.0 survives): densifying gives back
    `roll.astype(float32)` bit for bit."""
    x = roll.detach().cpu().numpy() if torch.is_tensor(roll) else np.asarray(roll)
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = x.view(np.uint32).reshape(-1, x.shape[-1])
    cells = np.flatnonzero(bits.any(axis=1))
    return SparseRoll(cells.astype(np.int32), x.reshape(bits.shape)[cells], x.shape, pin=pin)


_MODES = {'nonzero': _native.ROLL_NONZERO, 'hard': _native.ROLL_HARD}


def compact(x, mode='nonzero', pin=None, native=None):
    """Dense roll ON THE DEVICE (feature axis last) -> SparseRoll on the host, the inverse of `SparseRoll.to_dense`: the records
    are built on x's device by mst_roll_count / mst_roll_compact and only they are downloaded.  mode='nonzero': every cell with
    a non-zero bit pattern, features verbatim — `sparsify(x)`.  mode='hard': the cells hard_output (style/model.py:818-832)
    leaves with a non-zero velocity, carrying its hard features; `x` is not modified.  One 4-byte read of the count is the only
    synchronisation before the one copy of the records (into pinned memory when `pin`, default: for a GPU tensor).
    `native`: another build of the C ABI (tests: the CPU interpreter build, on CPU tensors)."""
    if mode not in _MODES:
        raise ValueError(f'mode {mode!r}: expected one of {sorted(_MODES)}')
    native = native or _native.get()
    shape = tuple(x.shape)
    x = x.detach()
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    nfeat = shape[-1] if len(shape) >= 2 else 0
    if nfeat not in (2, 5) or x.numel() == 0:
        raise ValueError(f'shape {shape}: the last axis holds the 5 pitched or 2 unpitched note features')
    n_cells = x.numel() // nfeat
    stream = _native.current_stream(x.device)
    ws = torch.empty(native.roll_slices(n_cells) + 1, dtype=torch.int32, device=x.device)
    native.roll_count(x, n_cells, nfeat, _MODES[mode], ws, stream)
    n = int(ws[-1])                                   # the only synchronisation: 4 bytes
    records = torch.empty(packed_words(n, nfeat), dtype=torch.int32, device=x.device)
    base = records.data_ptr() + 4 * HEADER
    native.roll_compact(x, n_cells, nfeat, _MODES[mode], ws, n, base, base + 4 * _cells_words(n), stream)
    if pin is None:
        pin = x.device.type == 'cuda'
    packed = torch.empty(records.numel(), dtype=torch.int32, pin_memory=bool(pin))
    packed.copy_(records)
    packed[:HEADER] = 0
    packed[0] = n
    packed[HEADER + n:HEADER + _cells_words(n)] = 0   # the padding behind the cells
    return SparseRoll.from_packed(packed, shape)


def stitch_records(rolls, bars):
    """The SparseRolls of consecutive `bars`-bar windows of one song, in order -> one SparseRoll of (1, C, n * bars, T, ...):
    the dense rolls concatenated along the bar axis, from the records.  Pure index arithmetic on the cells: a window's cell
    (c, r, j) becomes (c, w * bars + r, j) of the song; the result is sorted by cell like every SparseRoll."""
    rolls, bars = list(rolls), int(bars)
    if not rolls:
        raise ValueError('stitch_records: no windows')
    shape = tuple(rolls[0].shape)
    if len(shape) < 4 or shape[0] != 1 or shape[2] != bars or any(tuple(r.shape) != shape for r in rolls):
        raise ValueError(f'stitch_records: every window is a roll of (1, C, {bars}, T, ...), got {[tuple(r.shape) for r in rolls]}')
    per_bar = int(np.prod(shape[3:-1], dtype=np.int64))
    window, total = bars * per_bar, len(rolls) * bars * per_bar             # cells of one channel: in a window, in the song
    cells = []
    for w, roll in enumerate(rolls):
        c = roll.cells.numpy().astype(np.int64)
        cells.append(c // window * total + w * window + c % window)
    cells = np.concatenate(cells)
    order = np.argsort(cells, kind='stable')
    feats = np.concatenate([roll.feats.numpy() for roll in rolls])[order]
    return SparseRoll(cells[order].astype(np.int32), feats, shape[:2] + (len(rolls) * bars,) + shape[3:], pin=False)


def crop_bars(roll, n_bars):
    """The first `n_bars` bars of a SparseRoll of (1, C, R, T, ...): x[:, :, :n_bars] of the dense roll, from the records."""
    shape, n_bars = tuple(roll.shape), int(n_bars)
    if len(shape) < 4 or shape[0] != 1 or not 1 <= n_bars <= shape[2]:
        raise ValueError(f'crop_bars: {n_bars} bars of a roll of {shape}')
    per_bar = int(np.prod(shape[3:-1], dtype=np.int64))
    c = roll.cells.numpy().astype(np.int64)
    channel, rest = c // (shape[2] * per_bar), c % (shape[2] * per_bar)
    keep = rest < n_bars * per_bar
    cells = channel[keep] * (n_bars * per_bar) + rest[keep]
    return SparseRoll(cells.astype(np.int32), roll.feats.numpy()[keep], shape[:2] + (n_bars,) + shape[3:], pin=False)
