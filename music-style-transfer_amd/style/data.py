"""Host-side data pipeline with the reference's names (style/data.py:19-169): instrument vocabulary and
one-hot encoding, MIDI file -> model input (`iter_inputs`, `get_input`), `prepare_input`,
`get_used_instruments`.  Everything here runs on the host, per song; only `prepare_input` touches the
device (one H2D copy per tensor).  `prepare_input_sparse` is its counterpart for real songs: the note
tensors stay on the host as sorted note records (`SparseRoll`, `SparseClip`) and are expanded on the
device by mst_clip_scatter.  `SongStore` keeps the records of many songs on the device and `WindowBatch` names K equally
shaped windows of them (mst_clip_window crops them there) — append-only, or with `resident=N` a fixed ring that `admit` rotates
songs through (mst_store_admit); `StyleBank` keeps style vectors there.  sklearn's OneHotEncoder and pandas are not used: categories are the
sorted distinct values, which is what `categories='auto'` produces (style/data.py:23-27).
"""
import numpy as np
import torch

from style.exceptions import MidiFormatError
from style.midi import load_midi_from_file, is_pitched, program2instrument, program2group, popular_instruments
from style.midi_conversion import read_midi, ChannelConverter, NoteTable, _key_weights
from style.model import device
from style.scales import key_names, get_scale, major_mode
from style.sparse import SparseRoll, sparsify, compact # noqa: F401  (part of this module's surface)

included_instruments = popular_instruments
instrument_groups = [program2group[p] for p in included_instruments]
_instrument_categories = sorted(set(included_instruments))
_group_categories = sorted(set(instrument_groups))
n_instruments = len(included_instruments) + 1            # also percussion
instrument_size = len(_group_categories) + len(_instrument_categories)   # 51
percussion_id = len(included_instruments)
# per instrument logit (the order of _instrument_categories): the index of its GM family among _group_categories — what
# mst_info_decide needs to write encode_instruments' rows on the device
group_of_instrument = [_group_categories.index(program2group[p]) for p in _instrument_categories]


class CategoryOneHot:
    """The slice of sklearn's OneHotEncoder(sparse=False, categories='auto') the reference's callers use (style/data.py:23-27,
    124-125; style/style_transfer.py:115): `categories_`, `transform` of an (n, 1) column, `inverse_transform` of (n, k) rows."""

    def __init__(self, categories):
        self.categories_ = [np.array(categories)]
        self._index = {c: i for i, c in enumerate(categories)}

    def transform(self, column):
        column = np.asarray(column).reshape(-1)
        out = np.zeros((len(column), len(self._index)))
        for i, v in enumerate(column.tolist()):
            out[i, self._index[v]] = 1.
        return out

    def inverse_transform(self, rows):
        return self.categories_[0][np.asarray(rows).argmax(1)].reshape(-1, 1)


instruments_one_hot_encoder = CategoryOneHot(_instrument_categories)
groups_one_hot_encoder = CategoryOneHot(_group_categories)


def iter_all_midis(files, shuffle=False, looped=False):
    """(file, channels, info) of every readable file; unreadable files and MidiFormatErrors are skipped."""
    if shuffle:
        files = files[:]
        np.random.shuffle(files)
    while True:
        for file in files:
            mid = load_midi_from_file(file)
            if mid is None:
                continue
            try:
                channels, info = read_midi(mid)
            except MidiFormatError:
                continue
            yield file, channels, info
        if not looped:
            return


def iter_inputs(files, instruments, min_n_messages=100, *args, **kwargs):
    for filename, channels, info in iter_all_midis(files, *args, **kwargs):
        channels = [c for c in channels
                    if c['instrument_id'] in [-1, *instruments] and len(c['messages']) >= min_n_messages]
        if not any(is_pitched(c['instrument_id']) for c in channels):
            continue
        try:
            yield filename, get_input(channels, info)
        except Exception:
            print(filename)
            raise


def merge_nchannels(nchannels):
    """Channels playing the same instrument become one, notes ordered by onset (stable) (:103-114)."""
    instrument_ids = {n['instrument_id'] for n in nchannels}
    assert len(instrument_ids) == 1
    instrument_id = instrument_ids.pop()
    notes = NoteTable.concat([n['notes'] for n in nchannels])
    return {
        'channel_id': min(n['channel_id'] for n in nchannels),
        'instrument_id': instrument_id,
        'instrument_name': program2instrument[instrument_id],
        'notes': notes.take(np.argsort(notes.time, kind='stable')),
    }


def get_input(channels, info):
    """channels, info -> (info + detected scale, pitched rolls (C,R,T,10,56,5), instrument features
    (C,51), instrument ids, unpitched rolls (1,R,T,10,47,2) | None) (:66-100)."""
    cc = ChannelConverter(info)
    by_instrument = {}
    for channel in channels:
        by_instrument.setdefault(channel['instrument_id'], []).append(cc.channel2nchannel(channel))
    nchannels = [merge_nchannels(group) for group in by_instrument.values()]
    pitched = [n for n in nchannels if is_pitched(n['instrument_id'])]
    unpitched = [n for n in nchannels if not is_pitched(n['instrument_id'])]

    # seconds per pitch class: rows = keys, columns = channels; absent keys count 0 (DataFrame.sum skips NaN)
    seconds = np.zeros((len(key_names), len(pitched)))
    for j, nchannel in enumerate(pitched):
        weights, present = _key_weights(info, nchannel)
        seconds[present, j] = weights[present]
    keys_dist = seconds.sum(axis=1)
    keys_dist /= keys_dist.sum()
    info['scale'] = get_scale(keys_dist=keys_dist)

    pitched_vchannels = np.stack([cc.nchannel2vchannel(n) for n in pitched])
    unpitched_vchannels = np.stack([cc.nchannel2vchannel(n) for n in unpitched]) if unpitched else None
    instruments = [n['instrument_id'] for n in pitched]
    return info, pitched_vchannels, encode_instruments(instruments), instruments, unpitched_vchannels


def encode_instruments(instruments):
    """one-hot(program) ++ one-hot(GM family) per pitched channel -> (C, 51) float64 array."""
    x = np.zeros((len(instruments), instrument_size))
    for i, p in enumerate(instruments):
        x[i, _instrument_categories.index(p)] = 1.
        x[i, len(_instrument_categories) + _group_categories.index(program2group[p])] = 1.
    return x


def prepare_input(input, max_n_bars=None):
    """(filename, (info, pitched, instruments_features, instruments, unpitched)) -> device tensors
    (mode, bpm, pitched_channels, instruments_features, unpitched_channels), batch dim added."""
    _, (info, pitched_channels, instruments_features, _, unpitched_channels) = input
    if max_n_bars is None:
        max_n_bars = pitched_channels.shape[1]
    pitched_channels = torch.tensor(pitched_channels[:, :max_n_bars], dtype=torch.float).to(device).unsqueeze(0)
    instruments_features = torch.tensor(instruments_features, dtype=torch.float).to(device).unsqueeze(0)
    if unpitched_channels is not None:
        unpitched_channels = torch.tensor(unpitched_channels[:, :max_n_bars], dtype=torch.float).to(device).unsqueeze(0)
    is_major = info['scale']['mode'] in (major_mode, 'major')
    mode = torch.tensor([[1., 0.]] if is_major else [[0., 1.]]).to(device)
    bpm = torch.tensor(info['bpm'], dtype=torch.float).unsqueeze(0).to(device)
    return mode, bpm, pitched_channels, instruments_features, unpitched_channels


class SparseClip:
    """What `prepare_input` returns, kept on the host with the two note tensors as note records: `mode` (1, 2), `bpm` (1,),
    `pitched_channels` (SparseRoll of (1, C, R, T, 10, 56, 5)), `instruments_features` (1, C, 51), `unpitched_channels`
    (SparseRoll of (1, 1, R, T, 10, 47, 2) or None), and `bpm_target` (info['bpm'], the loss target).  The small tensors sit in
    pinned memory when a GPU is present (`pin`), so every upload of a clip is asynchronous.  Iterates like prepare_input's tuple."""

    def __init__(self, mode, bpm, pitched_channels, instruments_features, unpitched_channels, bpm_target=None, pin=None):
        self.pin = torch.cuda.is_available() if pin is None else bool(pin)

        def small(t):
            t = torch.as_tensor(t, dtype=torch.float32).cpu().contiguous()
            return t.pin_memory() if self.pin and not t.is_pinned() else t
        self.mode, self.bpm, self.instruments_features = small(mode), small(bpm), small(instruments_features)
        self.pitched_channels, self.unpitched_channels = pitched_channels, unpitched_channels
        self.bpm_target = float(self.bpm.reshape(-1)[0]) if bpm_target is None else bpm_target

    def __iter__(self):
        return iter((self.mode, self.bpm, self.pitched_channels, self.instruments_features, self.unpitched_channels))

    def drop_silent(self):
        """train-model.py:105-109 on the records: None for a clip without pitched notes; silent percussion removed."""
        if not self.pitched_channels.any():
            return None
        if self.unpitched_channels is not None and not self.unpitched_channels.any():
            return SparseClip(self.mode, self.bpm, self.pitched_channels, self.instruments_features, None, self.bpm_target, self.pin)
        return self

    def to_dense(self, device=device, native=None):
        """prepare_input's tuple of device tensors; the note tensors are built on the device by mst_clip_scatter."""
        up = lambda t: t.to(device, non_blocking=True)
        unpitched = None if self.unpitched_channels is None else self.unpitched_channels.to_dense(device, native=native)
        return (up(self.mode), up(self.bpm), self.pitched_channels.to_dense(device, native=native), up(self.instruments_features),
                unpitched)

    def save(self, path):
        """One .npz of the records and the small inputs (about 100 KB per song; the float64 rolls of a parsed song are tens
        of MB): a cache that spares parsing the MIDI file again."""
        items = dict(mode=self.mode.numpy(), bpm=self.bpm.numpy(), instruments_features=self.instruments_features.numpy(),
                     bpm_target=np.asarray(self.bpm_target))
        for key, roll in (('pitched', self.pitched_channels), ('unpitched', self.unpitched_channels)):
            if roll is not None:
                items.update({f'{key}_cells': roll.cells.numpy(), f'{key}_feats': roll.feats.numpy(),
                              f'{key}_shape': np.asarray(roll.shape, dtype=np.int64)})
        with open(path, 'wb') as f:              # (np.savez given a name appends '.npz' to it)
            np.savez_compressed(f, **items)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            roll = lambda key: SparseRoll(z[f'{key}_cells'], z[f'{key}_feats'], z[f'{key}_shape']) if f'{key}_cells' in z else None
            target = z['bpm_target'].item()
            return cls(z['mode'], z['bpm'], roll('pitched'), z['instruments_features'], roll('unpitched'), target)


class WindowBatch:
    """K windows of `bars` bars of one shape, as `SongStore.sample` draws them: clip k is bars [r0s[k], r0s[k] + bars) of song
    `songs[k]` of the store.  `C`, `T`, `percussion` are the bucket's; all K clips share them, so one batched plan runs them."""

    def __init__(self, C, bars, T, percussion, songs, r0s):
        self.C, self.bars, self.T, self.percussion = int(C), int(bars), int(T), bool(percussion)
        self.songs, self.r0s = np.asarray(songs, dtype=np.int64), np.asarray(r0s, dtype=np.int64)
        if self.songs.ndim != 1 or self.songs.shape != self.r0s.shape or not len(self.songs):
            raise ValueError('songs and r0s: two equally long 1-d lists, one entry per clip')

    @property
    def K(self):
        return len(self.songs)

    def __repr__(self):
        return (f'WindowBatch(C={self.C}, bars={self.bars}, T={self.T}, percussion={self.percussion}, '
                f'songs={self.songs.tolist()}, r0s={self.r0s.tolist()})')


class WindowList(list):
    """What `SongStore.windows` / `SongStore.window_batches` return: a list, with the number of windows the silence rule left
    out as `.skipped`."""
    skipped = 0


class _RecordPool:
    """The records of many songs back to back on the device: `cells` int32 (capacity,), `feats` float32 (capacity, nfeat)."""

    def __init__(self, nfeat, device, capacity):
        self.nfeat, self.used = nfeat, 0
        self.cells = torch.zeros(capacity, dtype=torch.int32, device=device)
        self.feats = torch.zeros(capacity, nfeat, dtype=torch.float32, device=device)

    def append(self, roll):
        """-> `first`: the roll's records are [first, first + roll.count) of the pool."""
        need = self.used + roll.count
        if need > self.cells.numel():
            _not_while_capturing(self.cells.device)
            capacity = self.cells.numel()
            while capacity < need:
                capacity *= 2
            cells, feats = self.cells.new_zeros(capacity), self.feats.new_zeros(capacity, self.nfeat)
            cells[:self.used].copy_(self.cells[:self.used])
            feats[:self.used].copy_(self.feats[:self.used])
            self.cells, self.feats = cells, feats         # (the old ones are recycled in stream order)
        first = self.used
        self.cells[first:need].copy_(roll.cells, non_blocking=True)
        self.feats[first:need].copy_(roll.feats, non_blocking=True)
        self.used = need
        return first


def _not_while_capturing(dev):
    if dev.type == 'cuda' and torch.cuda.is_current_stream_capturing():
        raise RuntimeError('SongStore: a device pool or table would have to grow while a stream is capturing; add the songs first')


class SongEvicted(LookupError):
    """A song id of a ring SongStore whose song has left the device."""


RING_ALIGN = 4            # records: a song's first record is a multiple of it, so cells (x 1) and feats (x 5, x 2) start on 16 bytes


def ring_place(head, count, capacity):
    """Where the next song of `count` records goes in a ring pool of `capacity` records whose head (the record behind the last
    placed song) is `head`: -> (first, new head).  `first` is `head` rounded up to a multiple of RING_ALIGN records, or 0 when
    the song would reach past the end from there.  Pure: says nothing about what lives at that place."""
    first = -(-int(head) // RING_ALIGN) * RING_ALIGN
    if first + count > capacity:
        first = 0
    return first, first + int(count)


def _up4(n):
    return -(-int(n) // 4) * 4


class SongStore:
    """Songs resident on the device, for training on windows of them (StyleTransferModel.train_windows).  `add` appends a
    song's pitched and unpitched note records to two device pools (grown by doubling, never during a capture) and its small
    inputs — mode, bpm, instrument features, used instruments, bpm target — as a row of a device table; the host keeps the
    cells, `(C, R, T)` and the percussion flag.  Songs are bucketed by `(C, T, has percussion)`: the windows of one bucket have
    one shape once their number of bars is chosen, which is what a batched plan needs.  `sample` draws K windows of a bucket;
    mst_clip_window crops them on the device, so no note data crosses the bus inside the training loop.

    `resident=N` makes the store a RING for training on more songs than fit: both pools hold exactly `capacity` records at
    addresses that never change, songs come in by `admit` — a group with one upload and one mst_store_admit launch — and the
    oldest leave to make room, so that at most N are resident.  Ids keep counting; `songs[id]` of an evicted song is None, and
    naming one raises SongEvicted.  Nothing a captured graph has baked in moves, so train_windows, eval_windows and transfer_*
    keep replaying across refreshes.  `resident=None` is the append-only store."""
    TRIES = 8             # windows tried per drawn song before another song is drawn
    STAGE_SLOTS = 4       # pinned blobs of `admit`, each reused only after the copy that last read it

    def __init__(self, device=device, capacity=1 << 14, resident=None):
        self.device = torch.device(device)
        self.songs = []                                   # per song id: dict of host-side facts
        self.pools = {n_feat: _RecordPool(n_feat, self.device, capacity) for n_feat in (5, 2)}
        self.buckets = {}                                 # (C, T, percussion) -> dict(songs, table, fields)
        self._silent = set()                              # (song, bars): no window of that many bars passes the silence rule
        self.resident_limit = None if resident is None else int(resident)
        if self.resident_limit is not None:
            if self.resident_limit < 1 or int(capacity) < 1:
                raise ValueError('SongStore: resident and capacity must be at least 1')
            self.capacity = int(capacity)
            self._live = []                               # resident ids, oldest first
            self._heads = {5: 0, 2: 0}
            self._stage = [dict(buf=None, done=None) for _ in range(self.STAGE_SLOTS)]
            self._stage_at = 0
            self._blob = self._status = None              # device staging buffer, status words (one row per launch)
            self._max_segments, self._launched = 64, []   # segments per launch of the last admit
            self.admit_native = None                      # a store on 'cpu' copies with torch unless given a style._native.Native

    def __len__(self):
        return len(self.songs)

    # ---- the ring
    def resident(self):
        """The ids of the songs on the device, oldest first."""
        if self.resident_limit is None:
            return list(range(len(self.songs)))
        return list(self._live)

    def evicted(self, song):
        return self.songs[song] is None

    def _song(self, song):
        s = self.songs[song]
        if s is None:
            raise SongEvicted(f'song {song} has left the store (SongStore.admit evicted it); draw the batch after the refresh')
        return s

    def _evict_oldest(self):
        song = self._live.pop(0)
        s, self.songs[song] = self.songs[song], None
        bucket = self.buckets[s['key']]
        bucket['songs'].remove(song)
        bucket['free'].append(s['row'])
        bucket['views'].pop(song, None)
        self._silent = {(i, bars) for i, bars in self._silent if i != song}

    def _overlaps(self, nfeat, first, count):
        name = 'pitched' if nfeat == 5 else 'unpitched'
        for song in self._live:
            at = self.songs[song][name]
            if at is not None and at[0] < first + count and first < at[0] + at[1]:
                return True
        return False

    def _bookkeeping(self):
        return dict(n=len(self.songs), songs={i: self.songs[i] for i in self._live}, live=list(self._live), heads=dict(self._heads),
                    silent=set(self._silent), keys=set(self.buckets),
                    buckets={key: (list(b['songs']), list(b['free']), dict(b['views']), b['table'], b['rows']) for key, b in self.buckets.items()})

    def _restore(self, was):
        del self.songs[was['n']:]
        for i, s in was['songs'].items():
            self.songs[i] = s
        self._live, self._heads, self._silent = was['live'], was['heads'], was['silent']
        for key in set(self.buckets) - was['keys']:
            del self.buckets[key]
        for key, (songs, free, views, table, rows) in was['buckets'].items():
            self.buckets[key].update(songs=songs, free=free, views=views, table=table, rows=rows)
        for nfeat, head in self._heads.items():
            self.pools[nfeat].used = head

    def admit(self, clips):
        """Take a group of SparseClips into a ring store (`resident=N`); returns their ids.  Silence is treated as in `add`, and a
        song whose pitched or unpitched records exceed `capacity` is refused (ValueError) — either before anything changes.  For
        each clip in turn the oldest resident songs are evicted until at most N are resident, the new one counted, and neither
        pool's place for it (`ring_place`) overlaps a live song.  The whole group then travels as ONE pinned blob — a header of
        segments, then per song its pitched cells and feats, unpitched cells and feats and its table row, every offset a
        multiple of 4 words — with one non-blocking copy into a device staging buffer and one mst_store_admit launch (more than
        one only when the group touches more than 12 buckets).

        Everything is enqueued on the CURRENT stream, which must be the stream the store's consumers (train_windows,
        eval_windows, transfer_*) run on: stream order is what keeps a crop that is still in flight from reading records this
        call overwrites.  After the launch nothing else is enqueued and nothing is waited for; `check` reads the status words
        where the caller synchronises anyway.  A WindowBatch drawn before this call may name evicted songs: it raises
        SongEvicted when used."""
        if self.resident_limit is None:
            raise ValueError('SongStore.admit: the store was made without resident=N; use add')
        from style import _native
        new = []
        for clip in clips:                                # refusals first: nothing has changed yet
            clip = clip.drop_silent()
            if clip is None:
                raise ValueError('SongStore.admit: a clip has no pitched notes (SparseClip.drop_silent() is None)')
            pitched, unpitched = clip.pitched_channels, clip.unpitched_channels
            _, C, R, T = pitched.shape[:4]
            if unpitched is not None and tuple(unpitched.shape[:4]) != (1, 1, R, T):
                raise ValueError(f'unpitched roll {unpitched.shape} does not match the pitched roll {pitched.shape}')
            if max(pitched.count, 0 if unpitched is None else unpitched.count) > self.capacity:
                raise ValueError(f'SongStore.admit: a song of {pitched.count} pitched and {0 if unpitched is None else unpitched.count} '
                                 f'unpitched records, the ring holds {self.capacity}')
            key = (C, T, unpitched is not None)
            used = get_used_instruments(clip.instruments_features, unpitched)
            parts = (clip.mode, clip.bpm, clip.instruments_features, used, torch.tensor([float(clip.bpm_target)]))
            row = torch.cat([t.reshape(-1).float() for t in parts])
            ends = np.cumsum([t.numel() for t in parts]).tolist()
            known = self.buckets.get(key)
            if known is not None and known['fields'][-1][1] != ends[-1]:
                raise ValueError(f'small inputs of {ends[-1]} floats, the bucket {key} holds rows of {known["fields"][-1][1]}')
            new.append((clip, key, row, ends))
        if not new:
            return []
        was = self._bookkeeping()
        try:
            ids = self._admit(new, _native)
        except BaseException:
            self._restore(was)
            raise
        return ids

    def _admit(self, new, _native):
        sounding = lambda roll: roll.cells.numpy()[np.any(roll.feats.numpy() != 0, axis=1)].astype(np.int64)
        ids, grown = [], set()
        for clip, key, row, ends in new:
            pitched, unpitched = clip.pitched_channels, clip.unpitched_channels
            rolls = [(5, pitched)] + ([(2, unpitched)] if unpitched is not None else [])
            while True:
                place = {nfeat: ring_place(self._heads[nfeat], roll.count, self.capacity) for nfeat, roll in rolls}
                if len(self._live) < self.resident_limit and not any(self._overlaps(nfeat, place[nfeat][0], roll.count)
                                                                      for nfeat, roll in rolls):
                    break
                self._evict_oldest()
            bucket = self.buckets.get(key)
            if bucket is None:
                # rows padded to 16 bytes: a row's copy is as aligned as the records'
                bucket = self.buckets[key] = dict(songs=[], fields=list(zip([0] + ends[:-1], ends)), views={}, free=[], rows=0,
                                                  table=torch.zeros(16, _up4(ends[-1]), dtype=torch.float32, device=self.device))
            if bucket['free']:
                at = bucket['free'].pop(0)
            else:
                at, bucket['rows'] = bucket['rows'], bucket['rows'] + 1
                if at == bucket['table'].shape[0]:
                    _not_while_capturing(self.device)
                    table = bucket['table'].new_zeros(2 * at, bucket['table'].shape[1])
                    table[:at].copy_(bucket['table'])
                    bucket['table'], bucket['views'] = table, {}
                    grown.add(key)
            C, R, T = key[0], pitched.shape[2], key[1]
            song = dict(C=C, R=R, T=T, percussion=unpitched is not None, key=key, row=at, pitched=(place[5][0], pitched.count),
                        pitched_cells=sounding(pitched), unpitched=None)
            if unpitched is not None:
                song.update(unpitched=(place[2][0], unpitched.count), unpitched_cells=sounding(unpitched))
            for nfeat, _ in rolls:
                self._heads[nfeat] = self.pools[nfeat].used = place[nfeat][1]
            self.songs.append(song)
            self._live.append(len(self.songs) - 1)
            bucket['songs'].append(len(self.songs) - 1)
            ids.append(len(self.songs) - 1)
        # the copies: of the group's songs that are still resident (a later member may have evicted an earlier one), so that
        # no two segments of a launch name the same words
        fixed = [self.pools[5].cells, self.pools[5].feats, self.pools[2].cells, self.pools[2].feats]
        todo = [(i, clip, row) for i, (clip, _, row, _) in zip(ids, new) if self.songs[i] is not None]
        launches, at = [], 0
        while at < len(todo):                             # groups of at most ADMIT_DSTS - 4 buckets
            keys, end = [], at
            while end < len(todo):
                key = self.songs[todo[end][0]]['key']
                if key not in keys:
                    if len(keys) == _native.ADMIT_DSTS - len(fixed):
                        break
                    keys.append(key)
                end += 1
            launches.append((keys, todo[at:end]))
            at = end
        packed = []
        for keys, part in launches:
            segments = []                                 # (dst, dst_off, the int32 words)
            for i, clip, row in part:
                s = self.songs[i]
                for slot, (name, roll) in enumerate((('pitched', clip.pitched_channels), ('unpitched', clip.unpitched_channels))):
                    if roll is None:
                        continue
                    first, nfeat = s[name][0], (5, 2)[slot]
                    segments.append((2 * slot, first, roll.cells.numpy().reshape(-1)))
                    segments.append((2 * slot + 1, first * nfeat, roll.feats.numpy().reshape(-1).view(np.int32)))
                table = self.buckets[s['key']]['table']
                segments.append((len(fixed) + keys.index(s['key']), s['row'] * table.shape[1], row.numpy().view(np.int32)))
            packed.append((fixed + [self.buckets[key]['table'] for key in keys], segments))
        self._reserve(max(len(segments) for _, segments in packed), max(sum(_up4(len(w)) for _, _, w in segments) for _, segments in packed),
                      len(packed))
        self._launched = []
        for n, (dsts, segments) in enumerate(packed):
            self._launch(n, dsts, segments, _native)
        return ids

    def _reserve(self, n_segments, payload_words, n_launches):
        """Room in the device staging buffer and the status words for launches of that size; they grow outside a capture only."""
        max_segments = self._max_segments
        while max_segments < n_segments:
            max_segments *= 2
        need = 4 + 4 * max_segments + payload_words
        if self._blob is None or max_segments > self._max_segments or need > self._blob.numel() or n_launches > self._status.shape[0]:
            _not_while_capturing(self.device)
            size = 1 << 12 if self._blob is None else self._blob.numel()
            while size < need:
                size *= 2
            self._max_segments = max_segments
            self._blob = torch.zeros(size, dtype=torch.int32, device=self.device)
            self._status = torch.zeros(n_launches, max_segments, dtype=torch.int32, device=self.device)

    def _launch(self, n, dsts, segments, _native):
        """One blob: packed into a pinned slot, uploaded, copied out on the device."""
        cuda = self.device.type == 'cuda'
        slot = self._stage[self._stage_at % len(self._stage)]
        self._stage_at += 1
        if slot['done'] is not None and not slot['done'].query():
            slot['done'].synchronize()
        if slot['buf'] is None or slot['buf'].numel() < self._blob.numel():
            _not_while_capturing(self.device)
            slot['buf'] = torch.zeros(self._blob.numel(), dtype=torch.int32, pin_memory=cuda)
        host = slot['buf'].numpy()
        host[:4] = (len(segments), 0, 0, 0)
        at = 4 + 4 * self._max_segments
        for k, (dst, dst_off, words) in enumerate(segments):
            host[4 + 4 * k:8 + 4 * k] = (dst, dst_off, at, len(words))
            host[at:at + len(words)] = words
            at += _up4(len(words))
        native = _native.get() if cuda else self.admit_native
        if native is None:                                # a store on the host: the same segments as torch copies
            for dst, dst_off, src_off, words in host[4:4 + 4 * len(segments)].reshape(-1, 4).tolist():
                dsts[dst].view(-1).view(torch.int32)[dst_off:dst_off + words].copy_(slot['buf'][src_off:src_off + words])
            self._status[n].zero_()
        else:
            self._blob[:at].copy_(slot['buf'][:at], non_blocking=True)
            if cuda:
                slot['done'] = slot['done'] or torch.cuda.Event()
                slot['done'].record()
            native.store_admit(self._blob, self._blob.numel(), self._max_segments, _native.AdmitDsts(dsts), self._status[n],
                               _native.current_stream(self.device))
        self._launched.append(len(segments))

    def check(self):
        """Download the status words of the last `admit` and raise if mst_store_admit refused a segment (it never does unless
        the bookkeeping here is wrong).  Synchronises: call it where the loop synchronises anyway."""
        if self.resident_limit is None or not self._launched:
            return
        status = self._status[:len(self._launched)].cpu()
        bad = [(n, k) for n, count in enumerate(self._launched) for k in np.flatnonzero(status[n].numpy()).tolist()]
        if bad:
            raise RuntimeError(f'SongStore.admit: mst_store_admit refused (launch, segment) {bad[:8]} of {self._launched} segments')

    def add(self, clip):
        """Take a SparseClip in; returns the song's id.  A clip whose percussion is silent is stored without it, as
        `SparseClip.drop_silent` would; one without pitched notes is refused (ValueError).  On a ring store: `admit([clip])[0]`."""
        if self.resident_limit is not None:
            return self.admit([clip])[0]
        clip = clip.drop_silent()
        if clip is None:
            raise ValueError('SongStore.add: the clip has no pitched notes (SparseClip.drop_silent() is None)')
        pitched, unpitched = clip.pitched_channels, clip.unpitched_channels
        _, C, R, T = pitched.shape[:4]
        if unpitched is not None and tuple(unpitched.shape[:4]) != (1, 1, R, T):
            raise ValueError(f'unpitched roll {unpitched.shape} does not match the pitched roll {pitched.shape}')
        key = (C, T, unpitched is not None)
        used = get_used_instruments(clip.instruments_features, unpitched)
        row = torch.cat([t.reshape(-1).float() for t in (clip.mode, clip.bpm, clip.instruments_features, used,
                                                         torch.tensor([float(clip.bpm_target)]))])
        bucket = self.buckets.get(key)
        if bucket is None:
            sizes = [clip.mode.numel(), clip.bpm.numel(), clip.instruments_features.numel(), used.numel(), 1]
            ends = np.cumsum(sizes).tolist()
            bucket = self.buckets[key] = dict(songs=[], fields=list(zip([0] + ends[:-1], ends)), views={},
                                              table=torch.zeros(16, ends[-1], dtype=torch.float32, device=self.device))
        if row.numel() != bucket['table'].shape[1]:
            raise ValueError(f'small inputs of {row.numel()} floats, the bucket {key} holds rows of {bucket["table"].shape[1]}')
        at = len(bucket['songs'])
        if at == bucket['table'].shape[0]:
            _not_while_capturing(self.device)
            table = bucket['table'].new_zeros(2 * at, row.numel())
            table[:at].copy_(bucket['table'])
            bucket['table'], bucket['views'] = table, {}
        bucket['table'][at].copy_(row)
        sounding = lambda roll: roll.cells.numpy()[np.any(roll.feats.numpy() != 0, axis=1)].astype(np.int64)
        song = dict(C=C, R=R, T=T, percussion=unpitched is not None, key=key, row=at,
                    pitched=(self.pools[5].append(pitched), pitched.count), pitched_cells=sounding(pitched), unpitched=None)
        if unpitched is not None:
            song.update(unpitched=(self.pools[2].append(unpitched), unpitched.count), unpitched_cells=sounding(unpitched))
        self.songs.append(song)
        bucket['songs'].append(len(self.songs) - 1)
        return len(self.songs) - 1

    def bucket_of(self, song):
        return self._song(song)['key']

    # ---- windows
    def window_sounds(self, song, r0, bars):
        """train-model.py:105-109 applied to a window: it holds a sounding pitched note and, for a song with percussion, a
        sounding unpitched one (a silent roll makes the loss's masked means 0 / 0).  Decided on the host cells."""
        s = self._song(song)
        per_bar = s['T'] * 10 * 56
        bounds = [(c * s['R'] + r0 + b) * per_bar for c in range(s['C']) for b in (0, bars)]
        at = np.searchsorted(s['pitched_cells'], bounds).reshape(-1, 2)
        if not np.any(at[:, 1] > at[:, 0]):
            return False
        if s['percussion']:
            per_bar = s['T'] * 10 * 47
            lo, hi = np.searchsorted(s['unpitched_cells'], [r0 * per_bar, (r0 + bars) * per_bar])
            return bool(hi > lo)
        return True

    def sample(self, rng, K, bars):
        """K windows of `bars` bars from ONE bucket -> WindowBatch, or None when no bucket can fill K slots.  The bucket is
        picked with probability proportional to its eligible songs (R >= bars); each slot draws a song uniformly from them and
        a first bar uniformly from [0, R - bars], keeps the window if `window_sounds`, tries up to 8 first bars and then
        draws another song.  `rng`: a numpy.random.Generator; the same generator state gives the same batch."""
        K, bars = int(K), int(bars)
        if K < 1 or bars < 1:
            raise ValueError('sample: K and bars must be at least 1')
        eligible = {key: [s for s in b['songs'] if self.songs[s]['R'] >= bars and (s, bars) not in self._silent]
                    for key, b in self.buckets.items()}
        while True:
            keys = [key for key in sorted(eligible) if eligible[key]]
            if not keys:
                return None
            weights = np.array([len(eligible[key]) for key in keys], dtype=np.float64)
            key = keys[int(rng.choice(len(keys), p=weights / weights.sum()))]
            songs, r0s = [], []
            pick = eligible[key]
            while pick and len(songs) < K:
                song = pick[int(rng.integers(len(pick)))]
                last = self.songs[song]['R'] - bars
                for _ in range(self.TRIES):
                    r0 = int(rng.integers(0, last + 1))
                    if self.window_sounds(song, r0, bars):
                        songs.append(song)
                        r0s.append(r0)
                        break
                else:
                    # eight misses: is there a window at all?  A song without one is not drawn again for this length
                    if not any(self.window_sounds(song, r0, bars) for r0 in range(last + 1)):
                        self._silent.add((song, bars))
                        pick.remove(song)
            if len(songs) == K:
                return WindowBatch(key[0], bars, key[1], key[2], songs, r0s)

    def windows(self, bars, stride=None):
        """The store's fixed set of windows of `bars` bars, for held-out evaluation: of every song with R >= bars the windows
        with first bar 0, stride, 2 * stride, ... <= R - bars (stride=None: `bars`, i.e. non-overlapping), as a list of
        (song id, first bar) — bucket by bucket (sorted keys), within a bucket in ascending song id, within a song in ascending
        first bar.  A window that fails `window_sounds` is left out; the list's `.skipped` says how many were.  No RNG: the
        same store gives the same list."""
        bars, stride = int(bars), int(bars if stride is None else stride)
        if bars < 1 or stride < 1:
            raise ValueError('windows: bars and stride must be at least 1')
        out = WindowList()
        for key in sorted(self.buckets):
            for song in sorted(self.buckets[key]['songs']):
                for r0 in range(0, self.songs[song]['R'] - bars + 1, stride):
                    if self.window_sounds(song, r0, bars):
                        out.append((song, r0))
                    else:
                        out.skipped += 1
        return out

    def window_batches(self, bars, K, stride=None):
        """`windows(bars, stride)` cut into batches of K for a `clips = K` plan: a list of (WindowBatch, live).  Each bucket's
        windows fill batches of their own (one shape per batch); a bucket's last batch is padded to K by repeating its last
        window, and `live` is the number of real windows in front.  `.skipped` is `windows`' count."""
        K = int(K)
        if K < 1:
            raise ValueError('window_batches: K must be at least 1')
        found = self.windows(bars, stride)
        out = WindowList()
        out.skipped = found.skipped
        by_bucket = {}
        for song, r0 in found:
            by_bucket.setdefault(self.songs[song]['key'], []).append((song, r0))
        for key in sorted(by_bucket):
            group = by_bucket[key]
            for at in range(0, len(group), K):
                part = group[at:at + K]
                live = len(part)
                part = part + [part[-1]] * (K - live)
                out.append((WindowBatch(key[0], bars, key[1], key[2], [s for s, _ in part], [r for _, r in part]), live))
        return out

    def describe(self, batch, out):
        """Fill `out` (a host int32 array (2, K, 4)) with the mst_window descriptors of the batch: row 0 for the pitched
        rolls, row 1 for the unpitched ones (zeros without percussion)."""
        rows = [(self._song(song), r0) for song, r0 in zip(batch.songs.tolist(), batch.r0s.tolist())]     # SongEvicted before a write
        out[:] = 0
        for k, (s, r0) in enumerate(rows):
            song = batch.songs[k]
            if s['key'] != (batch.C, batch.T, batch.percussion):
                raise ValueError(f'song {song} is of bucket {s["key"]}, the batch of {(batch.C, batch.T, batch.percussion)}')
            out[0, k] = (*s['pitched'], s['R'], r0)
            if s['percussion']:
                out[1, k] = (*s['unpitched'], s['R'], r0)

    def small_inputs(self, batch):
        """Views of the table rows of the batch's songs, clip by clip: mode, bpm, instrument features, used instruments, bpm
        target (the order of the plan's input slots)."""
        bucket = self.buckets[(batch.C, batch.T, batch.percussion)]
        views, out = bucket['views'], []
        facts = [self._song(song) for song in batch.songs.tolist()]
        for song, s in zip(batch.songs.tolist(), facts):
            if song not in views:
                row = bucket['table'][s['row']]
                views[song] = [row[a:b] for a, b in bucket['fields']]
            out += views[song]
        return out


class StyleBank:
    """Style vectors kept on the device, one row each: `rows` is a float32 tensor of `capacity` x `style_size`, grown by
    doubling and never during a capture (`_RecordPool`'s rule), of which the first `used` rows are taken.  Per row the host keeps
    where it came from — `provenance[row] = (song, first bar, bars)` — and per song its rows in the order they were taken
    (`by_song`).  A song is named by whatever the caller names it with (StyleTransferModel.encode_styles uses the SongStore's
    ids; a library that outlives the store does better with names); rows of every (channels, beats per bar, percussion) bucket
    share one bank, because a style vector does not depend on the bucket.

    A style to render with is a list of ENTRIES `(row, weight)`: `row(r)` is one stored style, `song(s)` the mean of a song's
    windows, `blend([...])` a weighted sum of such, and `StyleBank.mix` packs K of them as the CSR arrays mst_style_mix reads.
    Weights are float32 and products of them are rounded to float32, the arithmetic of the device.

    Every row has a GROUP, the ordinal of its song in `by_song`'s insertion order, so that a search can leave out a song's own
    rows (mst_style_search's groups / exclude).  The host keeps the groups as rows are taken; the device copy `groups` (int32, one
    per row of the capacity, sized and moved with `rows`) is refreshed at the next search, never during a capture."""

    def __init__(self, style_size, device=device, capacity=64):
        self.style_size, self.device = int(style_size), torch.device(device)
        if self.style_size < 1 or int(capacity) < 1:
            raise ValueError('StyleBank: style_size and capacity must be at least 1')
        self.rows = torch.zeros(int(capacity), self.style_size, dtype=torch.float32, device=self.device)
        self.groups = torch.full((int(capacity),), -1, dtype=torch.int32, device=self.device)
        self.used, self.provenance, self.by_song = 0, [], {}
        self._groups, self._group_of, self._groups_on_device, self._search = [], {}, 0, {}

    def __len__(self):
        return self.used

    @property
    def capacity(self):
        return self.rows.shape[0]

    def reserve(self, n):
        """Make room for `n` more rows (the tensor moves when it grows: never during a capture)."""
        need = self.used + int(n)
        if need > self.capacity:
            _not_while_capturing(self.device)
            capacity = self.capacity
            while capacity < need:
                capacity *= 2
            rows = self.rows.new_zeros(capacity, self.style_size)
            rows[:self.used].copy_(self.rows[:self.used])
            self.rows = rows                              # (the old one is recycled in stream order)
            self.groups = self.groups.new_full((capacity,), -1)
            self._groups_on_device = 0

    def take(self, song, r0, bars):
        """Name the next free row as the style of bars [r0, r0 + bars) of `song`; returns the row for whoever fills it."""
        self.reserve(1)
        row, self.used = self.used, self.used + 1
        self.provenance.append((song, int(r0), int(bars)))
        self._groups.append(self._group_of.setdefault(song, len(self._group_of)))
        self.by_song.setdefault(song, []).append(row)
        return row

    def add(self, song, r0, bars, style):
        """Store one style vector given as a tensor or array of style_size floats; returns its row."""
        style = torch.as_tensor(style, dtype=torch.float32).reshape(-1)
        if style.numel() != self.style_size:
            raise ValueError(f'StyleBank.add: a style of {style.numel()} floats, the bank holds rows of {self.style_size}')
        row = self.take(song, r0, bars)
        self.rows[row].copy_(style)
        return row

    def row(self, row):
        if not 0 <= int(row) < self.used:
            raise KeyError(f'StyleBank: row {row} of {self.used}')
        return [(int(row), np.float32(1.))]

    def song(self, song):
        """The mean of the song's windows: its rows, each with the weight float32(1) / float32(n)."""
        rows = self.by_song.get(song)
        if not rows:
            raise KeyError(f'StyleBank: no rows of song {song!r}')
        return [(r, np.float32(1.) / np.float32(len(rows))) for r in rows]

    def group_of(self, song):
        """The group of the song's rows — its ordinal among the bank's songs — or -1 for a song the bank does not hold."""
        return self._group_of.get(song, -1)

    def exclusions(self, nearest, songs):
        """Per clip of `songs` the group a search for `nearest` (a Nearest) leaves out: the song's own, or -1 — nothing — without
        exclude_own or for a song the bank does not hold.  ValueError when the bank holds fewer than nearest.k rows outside the
        largest excluded song: some clip would be left with a -1 among its rows."""
        groups = [self.group_of(song) if nearest.exclude_own else -1 for song in songs]
        most = max((len(self.by_song[song]) for song, g in zip(songs, groups) if g >= 0), default=0)
        if self.used - most < nearest.k:
            raise ValueError(f'{nearest!r} on a StyleBank of {self.used} rows, {most} of them of one excluded song: fewer than '
                             f'{nearest.k} rows are left to pick from')
        return groups

    def device_groups(self):
        """The device copy of the rows' groups, brought up to date (a copy of the rows taken since the last call: never during
        a capture)."""
        if self._groups_on_device < self.used:
            _not_while_capturing(self.device)
            new = torch.tensor(self._groups[self._groups_on_device:self.used], dtype=torch.int32)
            self.groups[self._groups_on_device:self.used].copy_(new)
            self._groups_on_device = self.used
        return self.groups

    def search(self, queries, k, exclude=None, farthest=False, native=None):
        """The `k` rows of the bank nearest to (or, with `farthest`, farthest from) each of Q query styles by cosine, ranked on
        the device by mst_style_search: -> (rows (Q, k) int32, scores (Q, k) float32) as numpy after one download; positions
        past the last rankable row hold -1 / NaN.  `queries` is a float32 tensor (Q, style_size) on the bank's device, or Q
        entry lists (`row`, `song`, `blend`), which mst_style_mix turns into a query buffer first.  `exclude`: Q song names or
        Nones; the rows of query q's song are left out for it (a song the bank does not hold leaves out nothing).  Only the
        first len(bank) rows are searched.  `native`: the library to call (default: the product library)."""
        from style import _native
        native = native or _native.get()
        k = int(k)
        if not 1 <= k <= _native.SEARCH_MAX_K:
            raise ValueError(f'StyleBank.search: k = {k}, not in [1, {_native.SEARCH_MAX_K}]')
        stream = _native.current_stream(self.device)
        if torch.is_tensor(queries):
            if queries.dim() != 2 or queries.shape[1] != self.style_size or queries.dtype != torch.float32 or queries.device != self.rows.device:
                raise ValueError(f'StyleBank.search: queries of {tuple(queries.shape)} {queries.dtype} on {queries.device}, not '
                                 f'(Q, {self.style_size}) float32 on {self.rows.device}')
            queries = queries.contiguous()
        else:
            offsets, idx, w = StyleBank.mix(queries)
            if len(idx) == 0:
                raise ValueError('StyleBank.search: no query')
            entries = [torch.from_numpy(a).to(self.device) for a in (offsets, idx, w)]
            queries = torch.empty(len(offsets) - 1, self.style_size, dtype=torch.float32, device=self.device)
            native.style_mix(self.rows, self.capacity, self.style_size, *entries, len(idx), queries, self.style_size, len(queries),
                             self.style_size, stream)
        Q = len(queries)
        if not 1 <= Q <= 4096:
            raise ValueError(f'StyleBank.search: {Q} queries, not in [1, 4096]')
        if exclude is not None and len(exclude) != Q:
            raise ValueError(f'StyleBank.search: {len(exclude)} exclusions for {Q} queries')
        groups = self.device_groups()
        small = torch.tensor([self.used] + [-1 if e is None else self.group_of(e) for e in (exclude or [None] * Q)], dtype=torch.int32)
        small = small.to(self.device)
        key = (self.capacity, Q, k)
        if key not in self._search:                             # (one scratch per shape in use; a grown bank drops the old ones)
            self._search = {s: t for s, t in self._search.items() if s[0] == self.capacity}
            self._search[key] = torch.empty(native.style_search_scratch_bytes(self.capacity, Q, k) // 8, dtype=torch.int64, device=self.device)
        rows = torch.empty(Q, k, dtype=torch.int32, device=self.device)
        scores = torch.empty(Q, k, dtype=torch.float32, device=self.device)
        native.style_search(self.rows, self.capacity, self.style_size, small[:1], groups, queries, Q, self.style_size, small[1:], self.style_size,
                            k, -1 if farthest else 1, rows, scores, self._search[key], stream)
        return rows.cpu().numpy(), scores.cpu().numpy()

    def song_means(self, native=None):
        """A new StyleBank on the same device with one row per song, in `by_song`'s order: the song's mean style, mixed on the
        device by mst_style_mix from `song(s)`; its provenance is (song, 0, the summed bars of the song's rows)."""
        from style import _native
        native = native or _native.get()
        means = StyleBank(self.style_size, self.device, capacity=max(len(self.by_song), 1))
        if not self.by_song:
            return means
        offsets, idx, w = StyleBank.mix([self.song(song) for song in self.by_song])
        for song, rows in self.by_song.items():
            means.take(song, 0, sum(self.provenance[r][2] for r in rows))
        entries = [torch.from_numpy(a).to(self.device) for a in (offsets, idx, w)]
        native.style_mix(self.rows, self.capacity, self.style_size, *entries, len(idx), means.rows, self.style_size, len(self.by_song),
                         self.style_size, _native.current_stream(self.device))
        return means

    def neighbours(self, song, k, farthest=False, native=None):
        """[(other song, cosine), ...]: the `k` songs whose mean style is nearest to (farthest from) the mean style of `song`,
        the song itself left out; fewer than k when the bank holds fewer other songs."""
        if song not in self.by_song:
            raise KeyError(f'StyleBank: no rows of song {song!r}')
        means = self.song_means(native)
        rows, scores = means.search([means.song(song)], k, exclude=[song], farthest=farthest, native=native)
        return [(means.provenance[r][0], float(s)) for r, s in zip(rows[0].tolist(), scores[0].tolist()) if r >= 0]

    def blend(self, parts):
        """[(what, weight), ...] -> the concatenated entries, each weight scaled (a float32 product).  `what` is a list of entries
        (from `row`, `song` or `blend`) or the name of a song; a single row goes in as `bank.row(r)`."""
        out = []
        for what, weight in parts:
            entries = what if isinstance(what, list) else self.song(what)
            out += [(int(r), np.float32(w) * np.float32(weight)) for r, w in entries]
        if not out:
            raise ValueError('StyleBank.blend: nothing to blend')
        return out

    @staticmethod
    def mix(styles):
        """K lists of entries -> the host CSR (offsets int32 (K + 1,), idx int32 (n,), w float32 (n,)) of mst_style_mix."""
        styles = [list(entries) for entries in styles]
        offsets = np.zeros(len(styles) + 1, dtype=np.int32)
        offsets[1:] = np.cumsum([len(entries) for entries in styles])
        idx = np.asarray([r for entries in styles for r, _ in entries], dtype=np.int32)
        w = np.asarray([x for entries in styles for _, x in entries], dtype=np.float32)
        return offsets, idx, w

    def save(self, path):
        """One .npz of the used rows and their provenance (song names as strings, with a flag for those that were ints), so that
        a style library outlives a session."""
        songs = [song for song, _, _ in self.provenance]
        if any(not isinstance(song, (int, np.integer, str)) for song in songs):
            raise ValueError('StyleBank.save: songs are named by ints or strings')
        with open(path, 'wb') as f:              # (np.savez given a name appends '.npz' to it)
            np.savez_compressed(f, rows=self.rows[:self.used].cpu().numpy(), songs=np.asarray([str(song) for song in songs], dtype=np.str_),
                                is_int=np.asarray([not isinstance(song, str) for song in songs], dtype=np.bool_),
                                r0=np.asarray([r0 for _, r0, _ in self.provenance], dtype=np.int64),
                                bars=np.asarray([bars for _, _, bars in self.provenance], dtype=np.int64))

    @classmethod
    def load(cls, path, device=device):
        with np.load(path) as z:
            rows = z['rows']
            bank = cls(rows.shape[1], device, capacity=max(len(rows), 1))
            for song, is_int, r0, bars in zip(z['songs'].tolist(), z['is_int'].tolist(), z['r0'].tolist(), z['bars'].tolist()):
                bank.take(int(song) if is_int else song, r0, bars)
            bank.rows[:len(rows)].copy_(torch.from_numpy(rows))
        return bank


class Nearest:
    """A `mix` for StyleTransferModel.transfer_styles that names no rows: every clip is rendered with the uniform blend (weights
    float32(1) / float32(k)) of the `k` rows of the bank whose cosine to the clip's own style is largest — or, with `farthest`,
    smallest — found on the device by mst_style_search.  `exclude_own`: rows of the clip's own song do not count."""

    def __init__(self, k=1, exclude_own=True, farthest=False):
        from style._native import SEARCH_MAX_K
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= SEARCH_MAX_K:
            raise ValueError(f'Nearest: k = {k!r}, not an int in [1, {SEARCH_MAX_K}]')
        self.k, self.exclude_own, self.farthest = int(k), bool(exclude_own), bool(farthest)

    @property
    def order(self):
        return -1 if self.farthest else 1

    def __repr__(self):
        return f'Nearest(k={self.k}, exclude_own={self.exclude_own}, farthest={self.farthest})'


def prepare_input_sparse(input, max_n_bars=None, pin=None):
    """`prepare_input` for the sparse input path: same cut to `max_n_bars`, same five items, but on the host — a SparseClip,
    in pinned memory when a GPU is present.  No device work; on a thread beside one that captures hipGraphs pass pin=False
    (allocating pinned memory is not allowed while any stream captures): the model then stages the records itself."""
    _, (info, pitched_channels, instruments_features, _, unpitched_channels) = input
    if max_n_bars is None:
        max_n_bars = pitched_channels.shape[1]
    pitched = sparsify(pitched_channels[:, :max_n_bars][None], pin=pin)
    unpitched = None if unpitched_channels is None else sparsify(unpitched_channels[:, :max_n_bars][None], pin=pin)
    is_major = info['scale']['mode'] in (major_mode, 'major')
    mode = torch.tensor([[1., 0.]] if is_major else [[0., 1.]])
    bpm = torch.tensor(info['bpm'], dtype=torch.float).unsqueeze(0)
    return SparseClip(mode, bpm, pitched, torch.tensor(instruments_features, dtype=torch.float).unsqueeze(0), unpitched,
                      bpm_target=info['bpm'], pin=pin)


def get_used_instruments(instruments_features, unpitched_channels):
    used = (instruments_features[:, :, :len(included_instruments)].sum(1) > 0).float()
    percussion = torch.tensor(unpitched_channels is not None, dtype=torch.float).to(used.device).view(1, 1)
    return torch.cat([used, percussion], 1)
