"""MI355X-native `style.model`: the reference's Python surface (style/model.py:28-997) over the HIP
hot path in libmst_amd.so.

What is kept, so that train-model.py:15-28,54-126 and style/style_transfer.py:17,67-131 run unchanged:
the nine module classes with their constructor signatures and the same `nn.Linear / nn.Conv1d /
LSTM / Distributed` children under the same attribute names (=> identical state_dict keys,
parameter order, seed-108 initialisation and pickle class paths), `StyleTransferModel` with
`extract_style / predict_song_info / apply_style / forward`, `get_total_loss` (including the
positional bpm-before-mode contract of train-model.py:115-122), `hard_output`, `device`.

What is different: no module executes torch ops.  The children are parameter containers; the
four model methods and the loss are `torch.autograd.Function`s that borrow `data_ptr()`s and
enqueue hand-written HIP kernels through the C ABI (include/mst_amd.h).  There is no CPU
fallback: without the library or without a GPU tensor the calls raise.
"""
import collections
import math

import numpy as np
import torch
from torch import nn

from style import _native
from style.sparse import SparseRoll, scatter_packed, compact
from style.utils.pytorch import Distributed, LSTM

epsilon = 1e-7
n_beat_fractions = 10
n_pitched_features = 5
n_unpitched_features = 2
n_octaves = 8
n_scale_degrees = 7
n_pitched_notes = n_octaves * n_scale_degrees
n_unpitched_notes = 47
n_modes = 2
min_bpm = 50
max_bpm = 200
bpm_range = max_bpm - min_bpm
mean_type = 'quadratic'
device = 'cuda' if torch.cuda.is_available() else 'cpu'

_DEFAULT_WIDTHS = dict(beat=64, bar=128, nrf=8, style=256, melody=8, rhythm=32, instr=51, n_instruments=41)
# Distributed(depth) of the wrapped children (style/model.py:53,68,119,467)
_DEPTH = {('pitched_channels_encoder', 'beats_conv'): 3, ('pitched_channels_encoder', 'beats_lstm'): 2,
          ('unpitched_channels_encoder', 'beats_lstm'): 2, ('song_info_model', 'beats_lstm'): 1}


def get_mean_size(*values, factor=1):
    return math.ceil(np.mean(values) * factor)


def _dims(C=1, R=1, T=1, unpitched=True, clips=0, **widths):
    w = dict(_DEFAULT_WIDTHS)
    w.update(widths)
    return _native.Dims(C=C, R=R, T=T, beat=w['beat'], bar=w['bar'], nrf=w['nrf'], style=w['style'], melody=w['melody'],
                        rhythm=w['rhythm'], instr=w['instr'], n_instruments=w['n_instruments'], has_unpitched=int(unpitched),
                        clips=clips)


class _Container(nn.Module):
    """A sub-module of the reference as a parameter container.  Children are created from the C
    ABI's parameter table (mst_param_info), in its order, so Python and HIP agree by construction."""
    _prefix = None

    def _build(self, **widths):
        self._widths = widths
        table = _native.get().param_table(_dims(**widths))
        groups = collections.OrderedDict()
        for name, _, shape in table:
            if not name.startswith(self._prefix + '.'):
                continue
            rest = name[len(self._prefix) + 1:]
            child, leaf = rest.split('.', 1)
            groups.setdefault(child, {})[leaf] = shape
        for child, leaves in groups.items():
            wrapped = any(k.startswith('module.') for k in leaves)
            leaves = {k[len('module.'):] if wrapped else k: v for k, v in leaves.items()}
            if 'weight_ih_l0' in leaves:
                four_h, n_in = leaves['weight_ih_l0']
                mod = LSTM(input_size=n_in, hidden_size=four_h // 4, num_layers=1, batch_first=True,
                           bidirectional='weight_ih_l0_reverse' in leaves)
            elif len(leaves['weight']) == 3:
                oc, ic, k = leaves['weight']
                mod = nn.Conv1d(in_channels=ic, out_channels=oc, kernel_size=k, stride=n_scale_degrees, padding=4)
            else:
                n_out, n_in = leaves['weight']
                mod = nn.Linear(in_features=n_in, out_features=n_out)
            if wrapped:
                mod = Distributed(mod, depth=_DEPTH[(self._prefix, child)])
            setattr(self, child, mod)

    def _owner(self):
        ref = self.__dict__.get('_parent')
        model = ref() if ref is not None else None
        if model is None:
            raise NotImplementedError(
                f'{type(self).__name__} is a parameter container on the MI355X path: its arithmetic is fused into the HIP kernels '
                'behind StyleTransferModel.extract_style / predict_song_info / apply_style / forward, and it can only be called '
                'on its own once it is part of a StyleTransferModel (the kernels need the whole flat parameter buffer).')
        return model

    def forward(self, *args, **kwargs):
        self._owner()
        raise NotImplementedError(
            f'{type(self).__name__}.forward takes intermediate tensors (beats / bars) that the fused plan does not accept as inputs; '
            'call StyleTransferModel.extract_style instead.  Stand-alone forwards exist for the channel encoders, SongInfoModel and '
            'the two style appliers (INTEGRATION.md section 2).')

    def __getstate__(self):          # the back-reference to the owning model is rebuilt by StyleTransferModel, never pickled
        d = dict(self.__dict__)
        d.pop('_parent', None)
        return d


def _named_slots(model, plan, names, shapes):
    return tuple(plan.view(n, s).clone() for n, s in zip(names, shapes))


class PitchedChannelsEncoder(_Container):
    _prefix = 'pitched_channels_encoder'

    def __init__(self, beat_size, bar_size, instrument_size):
        super().__init__()
        assert bar_size % 2 == 0
        self._build(beat=beat_size, bar=bar_size, instr=instrument_size)

    def forward(self, x, instruments_features):
        """style/model.py:77-99 on its own (forward only, no autograd): (beats (1,C,R,T,beat), bars (1,R,bar)).  Runs the
        extract stage of the owning model's plan and returns its named slots."""
        model = self._owner()
        with torch.no_grad():
            dev = model._anchor().device
            x = _f32c(x, dev)
            _, C, R, T = x.shape[:4]
            plan = model._plan(C, R, T, False, dev)
            plan.set_inputs(mode=torch.tensor([1., 0.]), bpm=torch.tensor([120.]), instr=_f32c(instruments_features, dev))
            plan.forward(_native.STAGE_EXTRACT, model._flat, x, None)
            return _named_slots(model, plan, ('pitched_beats', 'pitched_bars'), ((1, C, R, T, -1), (1, R, -1)))


class UnpitchedChannelsEncoder(_Container):
    _prefix = 'unpitched_channels_encoder'

    def __init__(self, beat_size, bar_size):
        super().__init__()
        assert bar_size % 2 == 0
        self._build(beat=beat_size, bar=bar_size)

    def forward(self, x):
        """style/model.py:128-141 on its own (forward only): (beats (1,1,R,T,beat), bars (1,R,bar)).  The plan needs a pitched
        tensor beside it; an all-zero single channel is supplied (the unpitched encoder does not read it)."""
        model = self._owner()
        with torch.no_grad():
            dev = model._anchor().device
            x = _f32c(x, dev)
            _, _, R, T = x.shape[:4]
            plan = model._plan(1, R, T, True, dev)
            pitched = torch.zeros(1, 1, R, T, n_beat_fractions, n_pitched_notes, n_pitched_features, device=dev)
            plan.set_inputs(mode=torch.tensor([1., 0.]), bpm=torch.tensor([120.]), instr=torch.zeros(1, model._widths.get('instr', 51)))
            plan.forward(_native.STAGE_EXTRACT, model._flat, pitched, x)
            return _named_slots(model, plan, ('unpitched_beats', 'unpitched_bars'), ((1, 1, R, T, -1), (1, R, -1)))


class StyleEncoder(_Container):
    _prefix = 'style_encoder'

    def __init__(self, style_size, bar_size, instrument_size):
        super().__init__()
        self._build(style=style_size, bar=bar_size, instr=instrument_size)


class MelodyEncoder(_Container):
    _prefix = 'melody_encoder'

    def __init__(self, melody_size, beat_size, bar_size, instrument_size):
        super().__init__()
        self._build(melody=melody_size, beat=beat_size, bar=bar_size, instr=instrument_size)


class PitchedRhythmEncoder(_Container):
    _prefix = 'pitched_rhythm_encoder'

    def __init__(self, rhythm_size, beat_size, bar_size, instrument_size):
        super().__init__()
        self._build(rhythm=rhythm_size, beat=beat_size, bar=bar_size, instr=instrument_size)


class UnpitchedRhythmEncoder(_Container):
    _prefix = 'unpitched_rhythm_encoder'

    def __init__(self, rhythm_size, beat_size, bar_size):
        super().__init__()
        self._build(rhythm=rhythm_size, beat=beat_size, bar=bar_size)


class SongInfoModel(_Container):
    _prefix = 'song_info_model'

    def __init__(self, n_rhythm_features, style_size, rhythm_size, n_instruments):
        super().__init__()
        self._build(nrf=n_rhythm_features, style=style_size, rhythm=rhythm_size, n_instruments=n_instruments)

    def forward(self, style, rhythm):
        """style/model.py:557-562 = StyleTransferModel.predict_song_info (differentiable)."""
        return self._owner().predict_song_info(style, rhythm)


class PitchedStyleApplier(_Container):
    _prefix = 'pitched_style_applier'

    def __init__(self, style_size, melody_size, rhythm_size, instrument_size):
        super().__init__()
        self._build(style=style_size, melody=melody_size, rhythm=rhythm_size, instr=instrument_size)

    def forward(self, style, melody, rhythm, instruments):
        """style/model.py:624-675 = the pitched half of StyleTransferModel.apply_style (differentiable)."""
        return self._owner().apply_style(style, melody, rhythm, instruments, unpitched=False)[0]


class UnpitchedStyleApplier(_Container):
    _prefix = 'unpitched_style_applier'

    def __init__(self, style_size, rhythm_size):
        super().__init__()
        self._build(style=style_size, rhythm=rhythm_size)

    def forward(self, style, rhythm):
        """style/model.py:703-724 (forward only): the unpitched half of apply_style; a zero melody and one blank instrument row
        stand in for the pitched applier's inputs, which this module does not read."""
        model = self._owner()
        with torch.no_grad():
            R, T = rhythm.shape[1:3]
            w = dict(_DEFAULT_WIDTHS); w.update(model._widths)
            melody = torch.zeros(1, R, T, n_beat_fractions, n_pitched_notes, w['melody'], device=rhythm.device)
            instr = torch.zeros(1, 1, w['instr'], device=rhythm.device)
            return model.apply_style(style, melody, rhythm, instr, unpitched=True)[1]


def _f32c(t, dev):
    return torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()


class StyleTransferModel(nn.Module):
    def __init__(self, pitched_channels_encoder, unpitched_channels_encoder, style_encoder, melody_encoder,
                 pitched_rhythm_encoder, unpitched_rhythm_encoder, song_info_model, pitched_style_applier,
                 unpitched_style_applier):
        super().__init__()
        self.pitched_channels_encoder = pitched_channels_encoder
        self.unpitched_channels_encoder = unpitched_channels_encoder
        self.style_encoder = style_encoder
        self.melody_encoder = melody_encoder
        self.pitched_rhythm_encoder = pitched_rhythm_encoder
        self.unpitched_rhythm_encoder = unpitched_rhythm_encoder
        self.song_info_model = song_info_model
        self.pitched_style_applier = pitched_style_applier
        self.unpitched_style_applier = unpitched_style_applier
        widths = {}
        for _, child in self.named_children():
            for k, v in child._widths.items():
                if widths.setdefault(k, v) != v:
                    raise ValueError(f'sub-modules disagree on {k}_size: {widths[k]} vs {v}')
        self._widths = widths
        self._link_children()
        # fail here, not at the first forward: the note-level HIP kernels exist for melody_size 4, 8, 12 and 16 only
        if _native.get().lib.mst_widths_supported(_dims(**widths)) != 0:
            raise _native.MstError(f'layer widths {widths} are outside the instantiated HIP kernels '
                                   '(melody_size must be a multiple of 4 from 4 to 16; LSTM hidden sizes <= 1024)')
        self._flat = self._gflat = None
        self._offsets = self._ends = self._slots = None
        self.graph_repeated_shapes = True       # train_iteration(): replay a hipGraph when a clip shape comes back

    def _link_children(self):
        import weakref
        for _, child in self.named_children():       # lets a sub-module be called on its own (see _Container.forward)
            child.__dict__['_parent'] = weakref.ref(self)

    def __setstate__(self, state):                   # whole-module snapshots (train-model.py:156-160): re-link after unpickling
        super().__setstate__(state)
        self._link_children()

    # ---- flat parameter / gradient buffers -------------------------------------------------
    def _sync_flat(self):
        """Point every Parameter's storage into ONE flat fp32 buffer laid out as the C ABI expects
        (model.parameters() order).  Re-done if the parameters moved (.to(), load_state_dict of new tensors)."""
        # fast path (every forward of a training loop): every Parameter OBJECT registered in the module tree is still the one
        # that was aliased into the flat buffer (identity against the leaf modules' own `_parameters` dicts: catches
        # load_state_dict(assign=True) and `module.weight = nn.Parameter(...)` anywhere in the tree, which install new objects
        # while the old ones keep aliasing the flat buffer), and the first and the last of them still point where they should
        # (catches .to(), which re-homes the data of all of them)
        ends = getattr(self, '_ends', None)
        slots = getattr(self, '_slots', None)
        if self._flat is not None and ends is not None and slots is not None:
            base = self._flat.data_ptr()
            if (all(reg.get(key) is p for reg, key, p in slots) and ends[0][0].data_ptr() == base + 4 * ends[0][1]
                    and ends[1][0].data_ptr() == base + 4 * ends[1][1]):
                return
        named = list(self.named_parameters())
        dev = named[0][1].device
        if dev.type != 'cuda':
            raise _native.MstError('the MI355X path needs the model on a GPU (model.to("cuda")); there is no CPU fallback')
        if self._flat is not None and self._flat.device == dev and all(
                p.data_ptr() == self._flat.data_ptr() + 4 * off for (_, p), off in zip(named, self._offsets)):
            self._ends = ((named[0][1], self._offsets[0]), (named[-1][1], self._offsets[-1]))
            self._slots = self._param_slots()
            return
        table = _native.get().param_table(_dims(**self._widths))
        if [n for n, _ in named] != [n for n, _, _ in table]:
            raise _native.MstError('parameter names/order differ from the C ABI layout')
        flat = torch.empty(_native.get().param_floats(_dims(**self._widths)), dtype=torch.float32, device=dev)
        for (name, p), (_, off, shape) in zip(named, table):
            if tuple(p.shape) != shape:
                raise _native.MstError(f'{name}: shape {tuple(p.shape)} != {shape}')
            flat[off:off + p.numel()].copy_(p.data.reshape(-1))
            p.data = flat[off:off + p.numel()].view(shape)
        self._flat, self._gflat = flat, torch.zeros_like(flat)
        self._offsets = [off for _, off, _ in table]
        self._ends = ((named[0][1], self._offsets[0]), (named[-1][1], self._offsets[-1]))
        self._slots = self._param_slots()

    def _param_slots(self):
        """(leaf module's `_parameters` dict, key, Parameter) for every parameter, in model.parameters() order."""
        return [(mod._parameters, key, p) for mod in self.modules() for key, p in mod._parameters.items() if p is not None]

    def _grad_target(self):
        """Where backward accumulates: the flat gradient buffer, aliased by every p.grad."""
        (p0, o0), (p1, o1) = self._ends            # fast path: first and last p.grad alias the flat gradient buffer
        gb = self._gflat.data_ptr()
        if p0.grad is not None and p1.grad is not None and p0.grad.data_ptr() == gb + 4 * o0 and p1.grad.data_ptr() == gb + 4 * o1:
            return self._gflat
        params = list(self.parameters())
        mine = [p.grad is not None and p.grad.data_ptr() == self._gflat.data_ptr() + 4 * off
                for p, off in zip(params, self._offsets)]
        if not any(p.grad is not None for p in params):
            self._gflat.zero_()             # zero_grad(set_to_none=True) dropped the aliases
        elif not all(mine):
            raise _native.MstError('p.grad was replaced by foreign tensors; use zero_grad() or keep the aliased grads')
        return self._gflat

    def _publish_grads(self):
        if self._ends[0][0].grad is not None and self._ends[1][0].grad is not None:
            return
        for p, off in zip(self.parameters(), self._offsets):
            if p.grad is None:
                p.grad = self._gflat[off:off + p.numel()].view(p.shape)

    def _plan(self, C, R, T, unpitched, dev, clips=0):
        return _native.get().plan(_dims(C=C, R=R, T=T, unpitched=unpitched, clips=clips, **self._widths), dev)

    def _anchor(self):
        self._sync_flat()
        return next(self.parameters())

    # ---- reference surface (style/model.py:751-793) ----------------------------------------
    # Grad mode is read HERE: inside autograd.Function.forward it is always off, so the Functions take it as a plain bool.
    def _dense(self, roll):
        """A note tensor given as a SparseRoll, densified on the model's device by mst_clip_scatter; anything else as it is."""
        return roll.to_dense(self._anchor().device) if isinstance(roll, SparseRoll) else roll

    def extract_style(self, mode, bpm, pitched_channels, instruments_features, unpitched_channels=None):
        pitched_channels, unpitched_channels = self._dense(pitched_channels), self._dense(unpitched_channels)
        return _Extract.apply(self, self._anchor(), torch.is_grad_enabled(), mode, bpm, pitched_channels, instruments_features,
                              unpitched_channels)

    def predict_song_info(self, style, rhythm):
        return _Predict.apply(self, self._anchor(), torch.is_grad_enabled(), style, rhythm)

    def apply_style(self, style, melody, rhythm, instruments_features, unpitched=False):
        x_pitched, x_unpitched = _Apply.apply(self, self._anchor(), torch.is_grad_enabled(), style, melody, rhythm,
                                              instruments_features, bool(unpitched))
        return x_pitched, (x_unpitched if unpitched else None)

    def train_iteration(self, mode, bpm, pitched_channels, instruments_features, unpitched_channels, used_instruments, bpm_target):
        """Opt-in fast form of one train-model.py loop body (train-model.py:113-126): forward, get_total_loss(normalize=True)
        with the inputs as targets, and loss.backward() in ONE C-ABI call (mst_train_iteration) — no autograd graph, no
        per-stage Python.  Gradients accumulate (sum) for optimizer.step() as usual.  Returns the 15 loss leaves as one device
        tensor (key order style._native.LOSS_KEYS; a row of a ring, valid for the next 256 calls of its lane).

        With `concurrent_accumulation` (FusedAdam switches it on) consecutive calls alternate between two LANES — two side
        streams, two workspaces per plan, two gradient buffers — so the iter_size = 2 accumulation iterations between two
        optimizer steps (train-model.py:95,151-153; they are independent: same parameters, gradients summed) overlap on the
        device; FusedAdam.step() joins the lanes and applies Adam to the sum of the two buffers (mst_adam_step2: bitwise what
        in-place accumulation gives).  p.grad shows lane 0's share until then."""
        anchor = self._anchor()
        dev = anchor.device
        # a note tensor may come as a SparseRoll (style.data): its records are uploaded on the lane's stream and
        # mst_clip_scatter writes the lane's static buffer directly, in place of the device-to-device copy of a dense tensor
        note = lambda t: t if t is None or isinstance(t, SparseRoll) else _f32c(t, dev)
        pitched, unpitched = note(pitched_channels), note(unpitched_channels)
        sparse = [t for t in (pitched, unpitched) if isinstance(t, SparseRoll)]
        new_buf = lambda t: None if t is None else torch.empty(tuple(t.shape), dtype=torch.float32, device=dev)
        _, C, R, T = pitched.shape[:4]
        plan = self._plan(C, R, T, unpitched is not None, dev)
        lanes = self._lanes(dev)
        li = 0
        if getattr(self, 'concurrent_accumulation', False):
            li = self._lane_next
            self._lane_next ^= 1
        lane = lanes[li]
        gflat = self._grad_target() if li == 0 else lane['grad']
        st = plan.__dict__.setdefault('_lane_state', {}).get(li)
        if st is None:
            st = plan._lane_state[li] = dict(ws=plan.ws if li == 0 else plan.new_ws(), graph=None, key=None, uses=0,
                                             pitched=new_buf(pitched), unpitched=new_buf(unpitched), records={},
                                             losses=torch.empty(_native.N_LOSSES, dtype=torch.float32, device=dev))
        ws = st['ws']
        small = [_f32c(mode, dev).reshape(-1), _f32c(bpm, dev).reshape(-1), _f32c(instruments_features, dev).reshape(-1),
                 _f32c(used_instruments, dev).reshape(-1),
                 torch.as_tensor(float(bpm_target), dtype=torch.float32).reshape(1).to(dev, non_blocking=True)]
        slots = [plan.view(n, ws=ws) for n in ('mode', 'bpm', 'instr', 'used_instruments', 'bpm_target')]
        cur = torch.cuda.current_stream(dev)
        side = lane['stream'] if li or getattr(self, 'concurrent_accumulation', False) else cur
        if side is not cur:
            side.wait_stream(cur)                      # the caller's inputs (and the last optimizer step) are ready
            for t in small + [t for t in (pitched, unpitched) if torch.is_tensor(t)]:
                t.record_stream(side)
        with torch.cuda.stream(side):
            # the note tensors are copied into the lane's static buffers unless the caller already wrote them there
            # (static_inputs()): a captured graph reads fixed addresses
            srcs, dsts = list(small), list(slots)
            if torch.is_tensor(pitched) and pitched.data_ptr() != st['pitched'].data_ptr():
                srcs.append(pitched.reshape(-1)); dsts.append(st['pitched'].reshape(-1))
            if torch.is_tensor(unpitched) and unpitched.data_ptr() != st['unpitched'].data_ptr():
                srcs.append(unpitched.reshape(-1)); dsts.append(st['unpitched'].reshape(-1))
            torch._foreach_copy_(dsts, srcs)           # one launch for all of them
            for roll in sparse:
                _scatter_records(roll, st['pitched'] if roll is pitched else st['unpitched'], st['records'], dev)
            # A shape seen before replays a hipGraph of the whole loop body (the launches of mst_train_iteration captured once
            # per plan and lane over static input buffers); songs of a new shape run eagerly.  Keyed by the buffers it baked in.
            key = (self._flat.data_ptr(), gflat.data_ptr())
            g = st['graph'] if st['key'] == key else None
            if g is None and st['uses'] >= 1 and dev.type == 'cuda' and getattr(self, 'graph_repeated_shapes', True):
                # (the plan has run eagerly before, so its code objects are loaded: capturing executes nothing and needs no warm-up)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side if side is not cur else None):
                    plan.train_iteration(self._flat, gflat, st['pitched'], st['unpitched'], st['losses'], ws=ws)
                st['graph'], st['key'] = g, key
            st['uses'] += 1
            if g is not None:
                plan._touch(ws)                         # a replay launches on this workspace
                g.replay()
            else:
                plan.train_iteration(self._flat, gflat, st['pitched'], st['unpitched'], st['losses'], ws=ws)
            ring = lane['ring']
            row = ring[lane['at'] % ring.shape[0]]
            lane['at'] += 1
            row.copy_(st['losses'])
        lane['dirty'] = True
        if li == 0:
            self._publish_grads()
        return row

    def eval_iteration(self, mode, bpm, pitched_channels, instruments_features, unpitched_channels, used_instruments, bpm_target):
        """One held-out evaluation of a song: train_iteration's forward and get_total_loss(normalize=True) with the inputs as
        targets, no backward, plus the note metrics of hard_output's decisions on the predictions — ONE C-ABI call
        (mst_eval_iteration).  The note tensors may be dense tensors or SparseRolls, exactly as for train_iteration.  Returns a
        style.metrics.EvalResult: `.losses` (the 15 leaves, key order style._native.LOSS_KEYS) and `.metrics` ((C + 2) x 8
        float64: the pitched channels, the unpitched roll — all zero without percussion — and the song info), both on the
        device; nothing is read back.  No reference counterpart: the reference has no validation.

        It runs on the current stream, behind whatever train_iteration has enqueued on its lanes (their bookkeeping is left
        alone), in a workspace and static note buffers of its own per plan: it touches no lane's workspace, no gradient
        buffer and not the lane counter, so the training it sits between is the same bits with or without it."""
        from style.metrics import EvalResult
        anchor = self._anchor()
        dev = anchor.device
        note = lambda t: t if t is None or isinstance(t, SparseRoll) else _f32c(t, dev)
        pitched, unpitched = note(pitched_channels), note(unpitched_channels)
        new_buf = lambda t: None if t is None else torch.empty(tuple(t.shape), dtype=torch.float32, device=dev)
        _, C, R, T = pitched.shape[:4]
        plan = self._plan(C, R, T, unpitched is not None, dev)
        st = plan.__dict__.get('_eval_state')
        if st is None:
            st = plan.__dict__['_eval_state'] = dict(ws=plan.new_ws(), pitched=new_buf(pitched), unpitched=new_buf(unpitched), records={})
        ws = st['ws']
        self.join_lanes_keep()
        srcs = [_f32c(mode, dev).reshape(-1), _f32c(bpm, dev).reshape(-1), _f32c(instruments_features, dev).reshape(-1),
                _f32c(used_instruments, dev).reshape(-1),
                torch.as_tensor(float(bpm_target), dtype=torch.float32).reshape(1).to(dev, non_blocking=True)]
        dsts = [plan.view(n, ws=ws) for n in ('mode', 'bpm', 'instr', 'used_instruments', 'bpm_target')]
        for t, buf in ((pitched, st['pitched']), (unpitched, st['unpitched'])):
            if torch.is_tensor(t):
                srcs.append(t.reshape(-1)); dsts.append(buf.reshape(-1))
        torch._foreach_copy_(dsts, srcs)
        for t, buf in ((pitched, st['pitched']), (unpitched, st['unpitched'])):
            if isinstance(t, SparseRoll):
                _scatter_records(t, buf, st['records'], dev)
        losses = torch.empty(_native.N_LOSSES, dtype=torch.float32, device=dev)
        metrics = torch.empty(C + 2, _native.METRIC_WORDS, dtype=torch.float64, device=dev)
        plan.eval_iteration(self._flat, st['pitched'], st['unpitched'], losses, metrics, ws=ws)
        return EvalResult(losses, metrics)

    def train_windows(self, store, batch):
        """K loop bodies in ONE batched pass: the K windows of `batch` (style.data.WindowBatch, drawn by `store.sample`) of the
        songs resident in `store` (style.data.SongStore, on the model's device) go through the `clips = K` plan of their shape.
        No note data is uploaded: the K window descriptors (16 bytes per clip and roll) travel as one copy from pinned memory,
        two mst_clip_window launches crop the windows out of the store's record pools into the plan's static note buffers,
        one _foreach_copy_ moves the clips' small inputs from the store's table into their workspace slots, and
        mst_train_iteration runs forward, loss and backward of all K clips.  The gradient of the K clips is ADDED to the
        model's gradient buffer (the sum over the clips, as K train_iteration calls would leave it), ready for
        optimizer.step().  Returns the K x 15 loss leaves (key order style._native.LOSS_KEYS) on the device; nothing is read
        back.  From the second use of a plan on, the two crops and the pass replay as one hipGraph: the descriptors are read
        on the device, so a replay serves other songs and other windows.

        It runs on the current stream, behind whatever train_iteration has enqueued on its lanes (their bookkeeping is left
        alone), in a workspace and note buffers of its own per plan: it touches neither lane 1's gradient buffer nor the lane
        counter."""
        anchor = self._anchor()
        dev = anchor.device
        if store.pools[n_pitched_features].cells.device != dev:
            raise _native.MstError(f'the SongStore lives on {store.device}, the model on {dev}')
        K, C, R, T, U = batch.K, batch.C, batch.bars, batch.T, batch.percussion
        plan = self._plan(C, R, T, U, dev, clips=K)
        st = plan.__dict__.get('_window_state')
        if st is None:
            ws = plan.new_ws()
            roll = lambda *shape: torch.empty((K,) + shape, dtype=torch.float32, device=dev)
            st = plan.__dict__['_window_state'] = dict(
                ws=ws, pitched=roll(C, R, T, n_beat_fractions, n_pitched_notes, n_pitched_features),
                unpitched=roll(1, R, T, n_beat_fractions, n_unpitched_notes, n_unpitched_features) if U else None,
                losses=torch.empty(K, _native.N_LOSSES, dtype=torch.float32, device=dev),
                win=torch.zeros(2, K, _native.WINDOW_WORDS, dtype=torch.int32, device=dev),
                # pinned staging slots of the descriptors, each reused only after the copy that last read it (its event)
                stage=[dict(buf=torch.zeros(2, K, _native.WINDOW_WORDS, dtype=torch.int32, pin_memory=dev.type == 'cuda'), done=None)
                       for _ in range(4)],
                slots=[plan.view(n, ws=ws, clip=k) for k in range(K)
                       for n in ('mode', 'bpm', 'instr', 'used_instruments', 'bpm_target')],
                at=0, graph=None, key=None, uses=0)
        ws = st['ws']
        self.join_lanes_keep()
        gflat = self._grad_target()
        stage = st['stage'][st['at'] % len(st['stage'])]
        st['at'] += 1
        if stage['done'] is not None and not stage['done'].query():
            stage['done'].synchronize()
        store.describe(batch, stage['buf'].numpy())
        st['win'].copy_(stage['buf'], non_blocking=True)
        if dev.type == 'cuda':
            stage['done'] = stage['done'] or torch.cuda.Event()
            stage['done'].record()
        torch._foreach_copy_(st['slots'], store.small_inputs(batch))
        pools = store.pools
        stream = _native.current_stream

        def body():
            native = _native.get()
            native.clip_window(pools[n_pitched_features].cells, pools[n_pitched_features].feats, st['win'][0], st['pitched'], K, C, R,
                               T * n_beat_fractions * n_pitched_notes, n_pitched_features, stream(dev))
            if U:
                native.clip_window(pools[n_unpitched_features].cells, pools[n_unpitched_features].feats, st['win'][1], st['unpitched'],
                                   K, 1, R, T * n_beat_fractions * n_unpitched_notes, n_unpitched_features, stream(dev))
            plan.train_iteration(self._flat, gflat, st['pitched'], st['unpitched'], st['losses'], ws=ws)

        # keyed by every address the capture bakes in: the parameters, the gradient buffer and the store's pools (they move
        # when they grow)
        key = (self._flat.data_ptr(), gflat.data_ptr()) + tuple(t.data_ptr() for p in pools.values() for t in (p.cells, p.feats))
        g = st['graph'] if st['key'] == key else None
        if g is None and st['uses'] >= 1 and dev.type == 'cuda' and getattr(self, 'graph_repeated_shapes', True):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            st['graph'], st['key'] = g, key
        st['uses'] += 1
        if g is not None:
            plan._touch(ws)
            g.replay()
        else:
            body()
        self._publish_grads()
        return st['losses'].clone()

    def eval_windows(self, store, batch, live=None, acc=None):
        """The forward-only twin of train_windows: the K windows of `batch` (style.data.WindowBatch) of the songs resident in
        `store` go through the `clips = K` plan of their shape as ONE evaluation pass — forward, get_total_loss(normalize=True)
        with the inputs as targets and the note metrics, no backward.  One copy from pinned memory carries the 2 K window
        descriptors, the K table rows of the clips' songs and `live` (9 K + 1 int32); then two mst_clip_window launches crop the
        windows (one without percussion), mst_window_inputs puts the clips' small inputs from the store's table into their
        workspace slots, mst_eval_iteration runs the pass and, when `acc` (style._native.EVAL_ACC_WORDS float64 on the model's
        device) is given, mst_eval_accumulate adds the first `live` clips (default: all K) into it — the rest of a padded batch
        is not scored.  From the second use of a plan on, that body replays as one hipGraph: descriptors, rows and `live` are
        read on the device, so a replay serves other songs, other windows and partial batches.  Returns (losses K x 15, metrics
        K x (C + 2) x 8 float64) of all K clips on the device; nothing is read back.

        It runs on the current stream, behind whatever train_iteration has enqueued on its lanes (their bookkeeping is left
        alone), in a workspace, note buffers and descriptors of its own per plan: it touches no gradient buffer, no lane, not
        the lane counter and not train_windows' state, so the training it sits between is the same bits with or without it."""
        anchor = self._anchor()
        dev = anchor.device
        if store.pools[n_pitched_features].cells.device != dev:
            raise _native.MstError(f'the SongStore lives on {store.device}, the model on {dev}')
        K, C, R, T, U = batch.K, batch.C, batch.bars, batch.T, batch.percussion
        live = K if live is None else int(live)
        if acc is not None and (acc.dtype != torch.float64 or acc.device != dev or not acc.is_contiguous()
                                or acc.numel() != _native.EVAL_ACC_WORDS):
            raise _native.MstError(f'eval_windows: acc must be {_native.EVAL_ACC_WORDS} contiguous float64 on {dev}')
        plan = self._plan(C, R, T, U, dev, clips=K)
        bucket = store.buckets[(C, T, U)]
        names = ('mode', 'bpm', 'instr', 'used_instruments', 'bpm_target')
        st = plan.__dict__.get('_eval_window_state')
        if st is None:
            n_desc = 2 * K * _native.WINDOW_WORDS
            roll = lambda *shape: torch.empty((K,) + shape, dtype=torch.float32, device=dev)
            fields = []
            for name, (a, b) in zip(names, bucket['fields']):
                off, _, numel = plan.slot(name)
                if numel != b - a:
                    raise _native.MstError(f'the store keeps {b - a} floats of {name}, the plan reads {numel}')
                fields.append((a, b - a, off))
            st = plan.__dict__['_eval_window_state'] = dict(
                ws=plan.new_ws(), pitched=roll(C, R, T, n_beat_fractions, n_pitched_notes, n_pitched_features),
                unpitched=roll(1, R, T, n_beat_fractions, n_unpitched_notes, n_unpitched_features) if U else None,
                losses=torch.empty(K, _native.N_LOSSES, dtype=torch.float32, device=dev),
                metrics=torch.empty(K, C + 2, _native.METRIC_WORDS, dtype=torch.float64, device=dev),
                # one int32 buffer: the 2 x K window descriptors, the K table rows, `live`
                desc=torch.zeros(n_desc + K + 1, dtype=torch.int32, device=dev), n_desc=n_desc,
                # pinned staging slots of that buffer, each reused only after the copy that last read it (its event)
                stage=[dict(buf=torch.zeros(n_desc + K + 1, dtype=torch.int32, pin_memory=dev.type == 'cuda'), done=None)
                       for _ in range(4)],
                fields=_native.RowFields.of(fields), at=0, graph=None, key=None, uses=0)
        ws, desc, n_desc = st['ws'], st['desc'], st['n_desc']
        self.join_lanes_keep()
        stage = st['stage'][st['at'] % len(st['stage'])]
        st['at'] += 1
        if stage['done'] is not None and not stage['done'].query():
            stage['done'].synchronize()
        host = stage['buf'].numpy()
        store.describe(batch, host[:n_desc].reshape(2, K, _native.WINDOW_WORDS))
        host[n_desc:n_desc + K] = [store.songs[s]['row'] for s in batch.songs.tolist()]
        host[n_desc + K] = live
        desc.copy_(stage['buf'], non_blocking=True)
        if dev.type == 'cuda':
            stage['done'] = stage['done'] or torch.cuda.Event()
            stage['done'].record()
        pools, table = store.pools, bucket['table']
        win = desc[:n_desc].view(2, K, _native.WINDOW_WORDS)
        stream = _native.current_stream

        def body():
            native = _native.get()
            native.clip_window(pools[n_pitched_features].cells, pools[n_pitched_features].feats, win[0], st['pitched'], K, C, R,
                               T * n_beat_fractions * n_pitched_notes, n_pitched_features, stream(dev))
            if U:
                native.clip_window(pools[n_unpitched_features].cells, pools[n_unpitched_features].feats, win[1], st['unpitched'],
                                   K, 1, R, T * n_beat_fractions * n_unpitched_notes, n_unpitched_features, stream(dev))
            # (the table's capacity, not its fill: a capture stays right while songs are added until the table moves)
            native.window_inputs(table, table.shape[0], table.shape[1], desc[n_desc:n_desc + K], K, st['fields'], plan.clip_stride,
                                 ws, stream(dev))
            plan.eval_iteration(self._flat, st['pitched'], st['unpitched'], st['losses'], st['metrics'], ws=ws)
            if acc is not None:
                native.eval_accumulate(st['losses'], st['metrics'], K, C, desc[n_desc + K:], acc, stream(dev))

        # keyed by every address the capture bakes in: the parameters, the store's pools and the bucket's table (they move when
        # they grow) and the accumulator
        key = (self._flat.data_ptr(), table.data_ptr(), None if acc is None else acc.data_ptr()) + \
            tuple(t.data_ptr() for p in pools.values() for t in (p.cells, p.feats))
        g = st['graph'] if st['key'] == key else None
        if g is None and st['uses'] >= 1 and dev.type == 'cuda' and getattr(self, 'graph_repeated_shapes', True):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            st['graph'], st['key'] = g, key
        st['uses'] += 1
        if g is not None:
            plan._touch(ws)
            g.replay()
        else:
            body()
        return st['losses'].clone(), st['metrics'].clone()

    def transfer_windows(self, store, batch, donors, score=False, capacity=None):
        """The inference twin of eval_windows: clip k of the K windows of `batch` (style.data.WindowBatch) of the songs resident
        in `store` is rendered with the style and the instruments of clip `donors[k]` of the same batch (K ints in [0, K); the
        identity gives reconstruction), decoded to note records on the device and, with `score`, scored there.  One copy from
        pinned memory carries the 2 K window descriptors, the K table rows of the clips' songs, the K rows of their donors'
        songs and the donors (11 K int32).  Then, as one chain on the `clips = K` plan of the batch's shape: two mst_clip_window
        launches crop the windows (one without percussion) and mst_window_inputs places each clip's own small inputs; the
        extract stage runs; two mst_clip_gather launches move the `style` vectors — into a bank of K x style_size floats, and
        back by `donors`; mst_window_inputs places the donors' small inputs (the info and apply stages read the instruments of
        them); the info and apply stages run; mst_rolls_count / mst_rolls_compact (MST_ROLL_HARD) turn the K predictions of each
        roll into note records, `capacity` per clip and roll (default min(n_cells, max(4096, n_cells // 8)) of the clip's roll).
        With `score`, mst_clip_scatter rebuilds from those records the rolls a written file holds (cells without a note are
        zero, unlike hard_output's dense result, which keeps their durations), mst_roll_metrics compares them with the clips' own
        notes (note retention), the extract stage runs on them with the donors' small inputs still in place — so the rendered
        style differs from the donor's through the notes alone — and mst_style_sums leaves the dot products of the rendered, the
        donor's and the own style (style.metrics.style_cosines).

        From the second use of a plan on, that body replays as one hipGraph per (score, capacity): descriptors, rows and donors
        are read on the device, so a replay serves other songs, other windows and other donors.  A donor outside [0, K) is not
        a Python error: the device writes NaNs into that clip's style (and reads no row), and the NaNs show in its predictions.
        Returns a style.metrics.TransferResult; its note records are on the host, downloaded after ONE synchronising read of
        the 2 K record counts.  A clip with more records than `capacity` raises MstError naming the capacity it needs: nothing
        is silently dropped.

        It runs on the current stream, behind whatever train_iteration has enqueued on its lanes (their bookkeeping is left
        alone), in a workspace, note buffers and descriptors of its own per plan: it touches no gradient buffer, no lane, not
        the lane counter and not the state of train_windows / eval_windows."""
        K = batch.K
        donors = np.asarray(donors, dtype=np.int64).reshape(-1)
        if len(donors) != K:
            raise ValueError(f'transfer_windows: {len(donors)} donors for a batch of {K} clips')
        donors = np.clip(donors, -2 ** 31, 2 ** 31 - 1)

        def fill(tail, own):                                    # the K donors' table rows, the K donors
            tail[:K] = [own[d] if 0 <= d < K else -1 for d in donors.tolist()]
            tail[K:] = donors

        def render(c):
            donor_rows, donor_idx = c.tail[:K], c.tail[K:]
            bank = c.st['bank']
            # the swap goes through the bank: permuting the slots in place would be a race
            c.native.clip_gather(c.style_slots, K, c.plan.clip_stride, bank, c.style_size, None, K, c.style_size, c.stream())
            c.native.clip_gather(bank, K, c.style_size, c.style_slots, c.plan.clip_stride, donor_idx, K, c.style_size, c.stream())
            c.native.window_inputs(c.table, c.table.shape[0], c.table.shape[1], donor_rows, K, c.st['fields'], c.plan.clip_stride, c.ws,
                                   c.stream())
            c.plan.forward(_native.STAGE_INFO | _native.STAGE_APPLY, self._flat, None, None, ws=c.ws)
            return K, donor_idx                                 # mst_style_sums: the bank's rows, and the row of a clip's target

        return self._transfer_pass('transfer_windows', lambda plan: (plan.__dict__, '_transfer_window_state'), store, batch, 2 * K, K,
                                   fill, render, (), score, capacity)

    def _transfer_pass(self, what, state_of, store, batch, tail, bank_rows, fill, render, key_extra, score, capacity, finish=None,
                       prepare=None):
        """The body transfer_windows and transfer_styles share: crops, own small inputs, the extract stage, `render` (whatever
        puts other styles and instruments in place and runs the info and apply stages; it returns the rows of st['bank'] and the
        device index of each clip's target row for mst_style_sums), the batched compaction and, with `score`, retention and the
        second extract; one upload of the descriptors, the own rows and `tail` further int32 that `fill(host tail, own rows)`
        writes; eager on a state's first use, one hipGraph per (score, capacities, key_extra) after it.  `state_of(plan)` names
        where the state lives: (a dict, its key)."""
        from types import SimpleNamespace
        from style.metrics import TransferResult
        anchor = self._anchor()
        dev = anchor.device
        if store.pools[n_pitched_features].cells.device != dev:
            raise _native.MstError(f'the SongStore lives on {store.device}, the model on {dev}')
        K, C, R, T, U = batch.K, batch.C, batch.bars, batch.T, batch.percussion
        native = _native.get()
        plan = self._plan(C, R, T, U, dev, clips=K)
        bucket = store.buckets[(C, T, U)]
        names = ('mode', 'bpm', 'instr', 'used_instruments', 'bpm_target')
        rolls = [(n_pitched_features, 'pitched', C, R * T * n_beat_fractions * n_pitched_notes)]
        if U:
            rolls.append((n_unpitched_features, 'unpitched', 1, R * T * n_beat_fractions * n_unpitched_notes))
        holder, state_key = state_of(plan)
        st = holder.get(state_key)
        if st is None:
            n_desc = 2 * K * _native.WINDOW_WORDS
            roll = lambda *shape: torch.empty((K,) + shape, dtype=torch.float32, device=dev)
            note_buffers = lambda: dict(pitched=roll(C, R, T, n_beat_fractions, n_pitched_notes, n_pitched_features),
                                        unpitched=roll(1, R, T, n_beat_fractions, n_unpitched_notes, n_unpitched_features) if U else None)
            fields = []
            for name, (a, b) in zip(names, bucket['fields']):
                off, _, numel = plan.slot(name)
                if numel != b - a:
                    raise _native.MstError(f'the store keeps {b - a} floats of {name}, the plan reads {numel}')
                fields.append((a, b - a, off))
            style_size = plan.slot('style')[2]
            st = holder[state_key] = dict(
                ws=plan.new_ws(), notes=note_buffers(), hard=note_buffers(),
                bank=torch.empty(bank_rows, style_size, dtype=torch.float32, device=dev),
                roll_ws={nfeat: torch.empty(K, native.roll_slices(ch * cells) + 1, dtype=torch.int32, device=dev) for nfeat, _, ch, cells in rolls},
                records={},                                     # capacity -> per roll (cells, feats), and the 2 K counts
                style_sums=torch.empty(K, _native.STYLE_SUM_WORDS, dtype=torch.float64, device=dev),
                retention=torch.zeros(K, C + 1, _native.METRIC_WORDS, dtype=torch.float64, device=dev),
                metrics={nfeat: (torch.empty(K * ch, _native.METRIC_WORDS, dtype=torch.float64, device=dev),
                                 torch.empty(native.roll_metrics_scratch_bytes(K * ch, cells) // 8, dtype=torch.float64, device=dev))
                         for nfeat, _, ch, cells in rolls},
                # one int32 buffer: the 2 x K window descriptors, the K own table rows, the caller's tail
                desc=torch.zeros(n_desc + K + tail, dtype=torch.int32, device=dev), n_desc=n_desc,
                # pinned staging slots of that buffer, each reused only after the copy that last read it (its event)
                stage=[dict(buf=torch.zeros(n_desc + K + tail, dtype=torch.int32, pin_memory=dev.type == 'cuda'), done=None)
                       for _ in range(4)],
                fields=_native.RowFields.of(fields), at=0, graphs={}, uses=0)
        ws, desc, n_desc = st['ws'], st['desc'], st['n_desc']
        if prepare is not None:
            prepare(st, plan)
        caps = tuple(min(ch * cells, max(4096, ch * cells // 8) if capacity is None else int(capacity)) for _, _, ch, cells in rolls)
        if min(caps) < 0:
            raise ValueError(f'{what}: capacity {capacity}')
        rec = st['records'].get(caps)
        if rec is None:
            rec = st['records'][caps] = dict(counts=torch.empty(2 * K, dtype=torch.int32, device=dev))
            for (nfeat, _, _, _), cap in zip(rolls, caps):
                rec[nfeat] = (torch.empty(K, max(cap, 1), dtype=torch.int32, device=dev),
                              torch.empty(K, max(cap, 1), nfeat, dtype=torch.float32, device=dev))
        self.join_lanes_keep()
        stage = st['stage'][st['at'] % len(st['stage'])]
        st['at'] += 1
        if stage['done'] is not None and not stage['done'].query():
            stage['done'].synchronize()
        host = stage['buf'].numpy()
        store.describe(batch, host[:n_desc].reshape(2, K, _native.WINDOW_WORDS))
        own = [store.songs[s]['row'] for s in batch.songs.tolist()]
        host[n_desc:n_desc + K] = own
        fill(host[n_desc + K:], own)
        desc.copy_(stage['buf'], non_blocking=True)
        if dev.type == 'cuda':
            stage['done'] = stage['done'] or torch.cuda.Event()
            stage['done'].record()
        pools, table = store.pools, bucket['table']
        win = desc[:n_desc].view(2, K, _native.WINDOW_WORDS)
        own_rows = desc[n_desc:n_desc + K]
        stream = _native.current_stream
        style_off, _, style_size = plan.slot('style')
        style_slots = ws.data_ptr() + 4 * style_off
        c = SimpleNamespace(native=native, plan=plan, st=st, ws=ws, tail=desc[n_desc + K:], table=table, style_slots=style_slots,
                            style_size=style_size, stream=lambda: stream(dev), dev=dev)   # (the stream is read inside a capture too)

        def body():
            notes, hard = st['notes'], st['hard']
            for nfeat, key, ch, cells in rolls:
                native.clip_window(pools[nfeat].cells, pools[nfeat].feats, win[0 if key == 'pitched' else 1], notes[key], K, ch, R,
                                   cells // R, nfeat, stream(dev))
            # (the table's capacity, not its fill: a capture stays right while songs are added until the table moves)
            native.window_inputs(table, table.shape[0], table.shape[1], own_rows, K, st['fields'], plan.clip_stride, ws, stream(dev))
            plan.forward(_native.STAGE_EXTRACT, self._flat, notes['pitched'], notes['unpitched'], ws=ws)
            sum_rows, sum_idx = render(c)
            for i, ((nfeat, key, ch, cells), cap) in enumerate(zip(rolls, caps)):
                x = ws.data_ptr() + 4 * plan.slot(key + '_pred')[0]
                out_cells, out_feats = rec[nfeat]
                counts = rec['counts'][i * K:(i + 1) * K]
                native.rolls_count(x, plan.clip_stride, K, ch * cells, nfeat, _native.ROLL_HARD, st['roll_ws'][nfeat], stream(dev))
                native.rolls_compact(x, plan.clip_stride, K, ch * cells, nfeat, _native.ROLL_HARD, st['roll_ws'][nfeat], cap, out_cells,
                                     out_feats, counts, stream(dev))
                if score:
                    native.clip_scatter(out_cells, out_feats, counts, hard[key], ch * cells, nfeat, n_clips=K, capacity=cap, stream=stream(dev))
                    records, scratch = st['metrics'][nfeat]
                    native.roll_metrics(hard[key], notes[key], K * ch, cells, nfeat, scratch, records, stream(dev))
                    at = slice(0, C) if key == 'pitched' else slice(C, C + 1)
                    st['retention'][:, at].copy_(records.view(K, ch, _native.METRIC_WORDS))
            if score:
                plan.forward(_native.STAGE_EXTRACT, self._flat, hard['pitched'], hard['unpitched'], ws=ws)
                native.style_sums(style_slots, plan.clip_stride, st['bank'], sum_rows, style_size, sum_idx, K, style_size, st['style_sums'],
                                  stream(dev))

        # keyed by every address the capture bakes in — the parameters, the store's pools and the bucket's table (they move when
        # they grow), the record buffers of this capacity — and by what the body does
        key = (self._flat.data_ptr(), table.data_ptr(), bool(score), caps) + tuple(key_extra) + \
            tuple(t.data_ptr() for p in pools.values() for t in (p.cells, p.feats))
        g = st['graphs'].get(key)
        if g is None and st['uses'] >= 1 and dev.type == 'cuda' and getattr(self, 'graph_repeated_shapes', True):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            st['graphs'][key] = g                               # (one per key in use: with and without score, per capacity)
        st['uses'] += 1
        if g is not None:
            plan._touch(ws)
            g.replay()
        else:
            body()
        rows_of = lambda name: torch.as_strided(ws, (K, plan.slot(name)[2]), (plan.clip_stride, 1), plan.slot(name)[0]).clone()
        result = TransferResult(rows_of('instruments_pred'), rows_of('mode_pred'), rows_of('bpm_pred').reshape(K), None, None,
                                st['style_sums'].clone() if score else None, st['retention'].clone() if score else None)
        if finish is not None:
            finish(c, result, rows_of)
        counts = rec['counts'].cpu().view(2, K)                 # the one synchronising read
        if not U:
            counts[1] = 0
        for i, ((nfeat, key, ch, cells), cap) in enumerate(zip(rolls, caps)):
            most = int(counts[i].max())
            if most > cap:
                raise _native.MstError(f'{what}: a clip has {most} {key} note records, the capacity is {cap}; '
                                       f'pass capacity={max(int(counts[:len(rolls)].max()), 1)}')
            out_cells, out_feats = rec[nfeat]
            host_cells, host_feats = out_cells[:, :most].cpu(), out_feats[:, :most].cpu()
            shape = (1, ch, R, T, n_beat_fractions, n_pitched_notes if key == 'pitched' else n_unpitched_notes, nfeat)
            setattr(result, key, [SparseRoll(host_cells[k, :n], host_feats[k, :n], shape, pin=False) for k, n in enumerate(counts[i].tolist())])
        return result

    def encode_styles(self, store, bars, K, stride=None, bank=None):
        """The style of every window of every song resident in `store`, kept on the device: for every batch of
        `store.window_batches(bars, K, stride)` — bucket by bucket — two mst_clip_window launches crop the windows,
        mst_window_inputs places the clips' small inputs, the extract stage of the `clips = K` plan runs and mst_style_put
        scatters the K `style` slots into rows of `bank` (a style.data.StyleBank; None: a new one) by a row list read on the
        device, -1 for the repeats that pad a bucket's last batch.  Songs of every bucket land in the one bank; the bank's
        provenance names each row's (song id of the store, first bar, bars).  Per plan the pass has a workspace, note buffers and
        descriptors of its own (not the lanes', not the other window states'); one copy from pinned memory carries descriptors,
        table rows and bank rows, and from the second use of a plan on the body replays as one hipGraph.  The rows for all
        windows are reserved before the first batch, so the bank does not move in between.  Nothing is downloaded.
        Returns the bank."""
        from style.data import StyleBank
        anchor = self._anchor()
        dev = anchor.device
        if store.pools[n_pitched_features].cells.device != dev:
            raise _native.MstError(f'the SongStore lives on {store.device}, the model on {dev}')
        todo = store.window_batches(bars, K, stride)
        K = int(K)
        w = dict(_DEFAULT_WIDTHS)
        w.update(self._widths)
        if bank is None:
            bank = StyleBank(w['style'], dev)
        if bank.style_size != w['style'] or bank.rows.device != dev:
            raise _native.MstError(f'encode_styles: a bank of {bank.style_size} floats per row on {bank.rows.device}, the model has '
                                   f'styles of {w["style"]} on {dev}')
        bank.reserve(sum(live for _, live in todo))
        native = _native.get()
        names = ('mode', 'bpm', 'instr', 'used_instruments', 'bpm_target')
        stream = _native.current_stream
        self.join_lanes_keep()
        for batch, live in todo:
            C, R, T, U = batch.C, batch.bars, batch.T, batch.percussion
            plan = self._plan(C, R, T, U, dev, clips=K)
            bucket = store.buckets[(C, T, U)]
            st = plan.__dict__.get('_encode_style_state')
            if st is None:
                n_desc = 2 * K * _native.WINDOW_WORDS
                roll = lambda *shape: torch.empty((K,) + shape, dtype=torch.float32, device=dev)
                fields = []
                for name, (a, b) in zip(names, bucket['fields']):
                    off, _, numel = plan.slot(name)
                    if numel != b - a:
                        raise _native.MstError(f'the store keeps {b - a} floats of {name}, the plan reads {numel}')
                    fields.append((a, b - a, off))
                st = plan.__dict__['_encode_style_state'] = dict(
                    ws=plan.new_ws(), pitched=roll(C, R, T, n_beat_fractions, n_pitched_notes, n_pitched_features),
                    unpitched=roll(1, R, T, n_beat_fractions, n_unpitched_notes, n_unpitched_features) if U else None,
                    # one int32 buffer: the 2 x K window descriptors, the K table rows, the K bank rows
                    desc=torch.zeros(n_desc + 2 * K, dtype=torch.int32, device=dev), n_desc=n_desc,
                    stage=[dict(buf=torch.zeros(n_desc + 2 * K, dtype=torch.int32, pin_memory=dev.type == 'cuda'), done=None)
                           for _ in range(4)],
                    fields=_native.RowFields.of(fields), at=0, graph=None, key=None, uses=0)
            ws, desc, n_desc = st['ws'], st['desc'], st['n_desc']
            stage = st['stage'][st['at'] % len(st['stage'])]
            st['at'] += 1
            if stage['done'] is not None and not stage['done'].query():
                stage['done'].synchronize()
            host = stage['buf'].numpy()
            store.describe(batch, host[:n_desc].reshape(2, K, _native.WINDOW_WORDS))
            host[n_desc:n_desc + K] = [store.songs[s]['row'] for s in batch.songs.tolist()]
            host[n_desc + K:] = -1
            for k, (song, r0) in enumerate(zip(batch.songs.tolist()[:live], batch.r0s.tolist()[:live])):
                host[n_desc + K + k] = bank.take(song, r0, R)
            desc.copy_(stage['buf'], non_blocking=True)
            if dev.type == 'cuda':
                stage['done'] = stage['done'] or torch.cuda.Event()
                stage['done'].record()
            pools, table, rows = store.pools, bucket['table'], bank.rows
            win = desc[:n_desc].view(2, K, _native.WINDOW_WORDS)
            style_off, _, style_size = plan.slot('style')

            def body():
                native.clip_window(pools[n_pitched_features].cells, pools[n_pitched_features].feats, win[0], st['pitched'], K, C, R,
                                   T * n_beat_fractions * n_pitched_notes, n_pitched_features, stream(dev))
                if U:
                    native.clip_window(pools[n_unpitched_features].cells, pools[n_unpitched_features].feats, win[1], st['unpitched'],
                                       K, 1, R, T * n_beat_fractions * n_unpitched_notes, n_unpitched_features, stream(dev))
                native.window_inputs(table, table.shape[0], table.shape[1], desc[n_desc:n_desc + K], K, st['fields'], plan.clip_stride,
                                     ws, stream(dev))
                plan.forward(_native.STAGE_EXTRACT, self._flat, st['pitched'], st['unpitched'], ws=ws)
                # (the bank's capacity, not its fill: a capture stays right while rows are taken until the bank moves)
                native.style_put(ws.data_ptr() + 4 * style_off, plan.clip_stride, rows, rows.shape[0], style_size, desc[n_desc + K:], K,
                                 style_size, stream(dev))

            # keyed by every address the capture bakes in: the parameters, the pools, the table and the bank (they move when they grow)
            key = (self._flat.data_ptr(), table.data_ptr(), rows.data_ptr(), rows.shape[0]) + \
                tuple(t.data_ptr() for p in pools.values() for t in (p.cells, p.feats))
            g = st['graph'] if st['key'] == key else None
            if g is None and st['uses'] >= 1 and dev.type == 'cuda' and getattr(self, 'graph_repeated_shapes', True):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    body()
                st['graph'], st['key'] = g, key
            st['uses'] += 1
            if g is not None:
                plan._touch(ws)
                g.replay()
            else:
                body()
        return bank

    def transfer_styles(self, store, batch, bank, mix, instruments='each', score=False, capacity=None, live=None):
        """transfer_windows with styles out of a bank: clip k of the K windows of `batch` is rendered with the weighted sum
        `mix` names for it of rows of `bank` (a style.data.StyleBank on the model's device) — a stored style, the mean of a
        song's windows, a blend of songs, a song of another (channels, beats per bar, percussion) bucket: a style vector does
        not depend on the bucket.  `mix` is StyleBank.mix's CSR (offsets, idx, w) or the K entry lists it is made of.
        `instruments` says what the clips play: 'each' — per clip the top C pitched instruments of its own instruments_pred,
        apply_style's rule (style.style_transfer.select_instruments), decided on the device by mst_info_decide together with the
        mode and the rounded tempo; 'pooled' — one such decision on the predictions summed over the first `live` clips (default
        all K), written to every clip, so that the windows of one file play the same instruments; or a float tensor of
        (1, C, 51) or (K, C, 51) instrument feature rows, placed as given (mode and tempo slots then stay the clips' own).

        The chain on the `clips = K` plan: the crops, the clips' own small inputs and the extract stage as in transfer_windows;
        mst_style_mix from the bank into the `style` slots; the info stage; mst_info_decide, or mst_clip_gather of the given
        rows into the `instr` slots; the apply stage; mst_rolls_count / mst_rolls_compact.  With `score` the own styles and the
        mixed targets are kept in one side buffer of 2 K rows, so that mst_style_sums scores the rendered style against target
        row K + k and own row k; the second extract reads the decided mode, tempo and instruments; note retention is
        transfer_windows'.  One copy from pinned memory carries the descriptors, the table rows and the CSR.  The CSR has an
        entry capacity per state (the next power of two, at least 4 K): more entries than a state holds means another state,
        never a silent cut.  From a state's second use on the body replays as one hipGraph per (score, capacity, instruments
        kind, entry capacity): rows, offsets, indices, weights and `live` are read on the device, so a replay serves other
        windows and other mixes.  A clip whose entries are empty or name a row outside the bank gets NaNs for a style, which
        show in its predictions; rows at or beyond len(bank) but inside its capacity are not checked.

        `mix` may also be a style.data.Nearest(k, exclude_own, farthest): no rows are named, and behind the extract stage
        mst_style_search ranks the clips' own styles (the K `style` slots, the plan's clip stride apart) against the first
        len(bank) rows and writes the k nearest (farthest) rows of every clip into the CSR's idx on the device; offsets are
        arange(K + 1) k and every weight float32(1) / float32(k), so the chain goes on unchanged with the uniform blend of the
        neighbours, in the same graph and with no host round trip.  With `exclude_own` the rows of the clip's own song (its group
        in the bank) do not count.  ValueError when the bank holds fewer than k rows outside the largest excluded song, so
        that no clip is left with a -1 among its rows.  The result then carries `neighbours` and `neighbour_scores` (K, k).

        Returns a style.metrics.TransferResult with `instr_features` (K, C, 51) and, where the device decided, `decisions`
        (K, C + 2 int32).  What transfer_windows says about streams, lanes and the training state holds here: the states are
        this method's own."""
        from style.data import Nearest, StyleBank, group_of_instrument
        K, C = batch.K, batch.C
        dev = self._anchor().device
        if bank.rows.device != dev:
            raise _native.MstError(f'the StyleBank lives on {bank.rows.device}, the model on {dev}')
        nearest = mix if isinstance(mix, Nearest) else None
        exclude = np.full(K, -1, dtype=np.int32)
        if nearest is not None:
            exclude[:] = bank.exclusions(nearest, batch.songs.tolist())
            # the search fills idx on the device; offsets and weights are the uniform blend of k rows per clip
            mix = (np.arange(K + 1) * nearest.k, np.full(K * nearest.k, -1), np.full(K * nearest.k, np.float32(1.) / np.float32(nearest.k)))
            groups = bank.device_groups()                       # (brought up to date here: never during a capture)
        offsets, idx, w = mix if isinstance(mix, tuple) and len(mix) == 3 and not isinstance(mix[0], list) else StyleBank.mix(mix)
        offsets, idx = np.asarray(offsets, dtype=np.int32).reshape(-1), np.asarray(idx, dtype=np.int32).reshape(-1)
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1))
        if len(offsets) != K + 1 or len(idx) != len(w):
            raise ValueError(f'transfer_styles: a mix of {len(offsets) - 1} clips and {len(idx)} / {len(w)} entries for a batch of {K}')
        n_entries = len(idx)
        entry_cap = 4 * K
        while entry_cap < n_entries:
            entry_cap *= 2
        given = None
        if torch.is_tensor(instruments):
            given = instruments.to(dev, torch.float32)
            kind = 'given'
            if given.dim() != 3 or given.shape[0] not in (1, K) or given.shape[1] != C:
                raise ValueError(f'transfer_styles: instruments of {tuple(instruments.shape)}, not (1 or {K}, {C}, instrument features)')
        elif instruments in ('each', 'pooled'):
            kind = instruments
        else:
            raise ValueError(f"transfer_styles: instruments is 'each', 'pooled' or a tensor, not {instruments!r}")
        live = K if live is None else int(live)
        at_off, at_live, at_idx, at_w = K, 2 * K + 1, 2 * K + 2, 2 * K + 2 + entry_cap      # the tail: targets, offsets, live, idx, w,
        at_ex, at_used = at_w + entry_cap, at_w + entry_cap + K                             # the clips' excluded groups, len(bank)

        def fill(tail, own):
            tail[:K] = np.arange(K, 2 * K)                      # mst_style_sums: clip k's target is row K + k of the side buffer
            tail[at_off:at_off + K + 1] = offsets
            tail[at_live] = live
            tail[at_idx:at_idx + n_entries] = idx
            tail[at_idx + n_entries:at_w] = -1
            tail[at_w:at_w + n_entries] = w.view(np.int32)
            tail[at_w + n_entries:at_ex] = 0
            tail[at_ex:at_used] = exclude
            tail[at_used] = len(bank)

        def render(c):
            plan, ws, native, st = c.plan, c.ws, c.native, c.st
            side, rows = st['bank'], bank.rows
            slot = lambda name: ws.data_ptr() + 4 * plan.slot(name)[0]
            if score:                                           # the own styles: rows [0, K) of the side buffer
                native.clip_gather(c.style_slots, K, plan.clip_stride, side, c.style_size, None, K, c.style_size, c.stream())
            # (the bank's capacity, not its fill: a capture stays right while rows are added until the bank moves)
            if nearest is not None:                             # the clips' own styles are the queries; the rows land in idx
                native.style_search(rows, rows.shape[0], c.style_size, c.tail[at_used:], groups, c.style_slots, K, plan.clip_stride,
                                    c.tail[at_ex:], c.style_size, nearest.k, nearest.order, c.tail[at_idx:], st['neighbour_scores'],
                                    st['search_scratch'][(rows.shape[0], nearest.k)], c.stream())
            native.style_mix(rows, rows.shape[0], c.style_size, c.tail[at_off:], c.tail[at_idx:], c.tail[at_w:].view(torch.float32),
                             entry_cap, c.style_slots, plan.clip_stride, K, c.style_size, c.stream())
            if score:                                           # the mixed targets: rows [K, 2 K)
                native.clip_gather(c.style_slots, K, plan.clip_stride, side[K:], c.style_size, None, K, c.style_size, c.stream())
            plan.forward(_native.STAGE_INFO, self._flat, None, None, ws=ws)
            row = plan.slot('instr')[2]
            if given is None:
                n_logits = plan.slot('instruments_pred')[2]
                native.info_decide(slot('instruments_pred'), slot('mode_pred'), slot('bpm_pred'), plan.clip_stride, n_logits,
                                   group_of_instrument, row // C - (n_logits - 1), C, K, kind == 'pooled', c.tail[at_live:], slot('instr'),
                                   slot('mode'), slot('bpm'), plan.clip_stride, st['decisions'], c.stream())
            else:
                native.clip_gather(st['given'], K, row if given.shape[0] == K else 0, slot('instr'), plan.clip_stride, None, K, row,
                                   c.stream())
            plan.forward(_native.STAGE_APPLY, self._flat, None, None, ws=ws)
            return 2 * K, c.tail[:K]

        def state_of(plan):
            return plan.__dict__.setdefault('_transfer_style_state', {}), entry_cap

        def prepare(st, plan):                                  # buffers a state of this method owns beside the shared ones
            if 'decisions' not in st:
                st['decisions'] = torch.zeros(K, C + 2, dtype=torch.int32, device=dev)
                st['given'] = torch.zeros(K, plan.slot('instr')[2], dtype=torch.float32, device=dev)
            if given is not None:
                if given[0].numel() != plan.slot('instr')[2]:
                    raise ValueError(f'transfer_styles: instrument rows of {given[0].numel()} floats, the plan reads {plan.slot("instr")[2]}')
                st['given'][:given.shape[0]].copy_(given.reshape(given.shape[0], -1))
            if nearest is not None:
                if 'neighbour_scores' not in st:
                    st['neighbour_scores'] = torch.zeros(K * _native.SEARCH_MAX_K, dtype=torch.float32, device=dev)
                    st['search_scratch'] = {}
                shape = (bank.rows.shape[0], nearest.k)
                if shape not in st['search_scratch']:
                    st['search_scratch'][shape] = torch.empty(_native.get().style_search_scratch_bytes(shape[0], K, nearest.k) // 8,
                                                              dtype=torch.int64, device=dev)

        def finish(c, result, rows_of):
            result.instr_features = rows_of('instr').view(K, C, -1)
            result.decisions = c.st['decisions'].clone() if given is None else None
            if nearest is not None:
                result.neighbours = c.tail[at_idx:at_idx + n_entries].view(K, nearest.k).clone()
                result.neighbour_scores = c.st['neighbour_scores'][:n_entries].view(K, nearest.k).clone()

        key_extra = (kind, entry_cap, bank.rows.data_ptr(), bank.rows.shape[0], None if given is None else given.shape[0])
        if nearest is not None:
            key_extra += (('nearest', nearest.k, nearest.order, nearest.exclude_own), groups.data_ptr())
        return self._transfer_pass('transfer_styles', state_of, store, batch, at_used + 1, 2 * K, fill, render, key_extra, score,
                                   capacity, finish=finish, prepare=prepare)

    def eval_accumulator(self):
        """The model's accumulator of evaluation rounds (style.train.evaluate_windows): EVAL_ACC_WORDS float64 on the model's
        device, allocated once, so that the graphs of eval_windows bake in one address."""
        dev = self._anchor().device
        acc = self.__dict__.get('_eval_acc')
        if acc is None or acc.device != dev:
            acc = self.__dict__['_eval_acc'] = torch.zeros(_native.EVAL_ACC_WORDS, dtype=torch.float64, device=dev)
        return acc

    def static_inputs(self, C, R, T, unpitched=True, lane=0):
        """The note-tensor buffers a captured train_iteration of this shape reads (created on first use by train_iteration): a
        loader that writes its H2D copies straight into them saves the per-iteration device copy."""
        plan = self._plan(C, R, T, unpitched, self._anchor().device)
        st = plan.__dict__.get('_lane_state', {}).get(lane)
        return (st['pitched'], st['unpitched']) if st else None

    def _lanes(self, dev):
        lanes = self.__dict__.get('_lane_list')
        if lanes is None or lanes[0]['ring'].device != dev:
            mk = lambda: dict(stream=torch.cuda.Stream(dev) if dev.type == 'cuda' else None, grad=None, dirty=False, at=0,
                              ring=torch.zeros(256, _native.N_LOSSES, dtype=torch.float32, device=dev))
            lanes = self.__dict__['_lane_list'] = [mk(), mk()]
            lanes[1]['grad'] = torch.zeros_like(self._flat)
            self.__dict__['_lane_next'] = 0
        if lanes[1]['grad'].data_ptr() == 0 or lanes[1]['grad'].numel() != self._flat.numel() or lanes[1]['grad'].device != self._flat.device:
            lanes[1]['grad'] = torch.zeros_like(self._flat)
        return lanes

    def join_lanes(self):
        """Make the current stream wait for everything train_iteration has enqueued on its lanes; returns lane 1's gradient
        buffer if it holds a share of the accumulated gradient (else None).  FusedAdam.step and LossLog.flush call it."""
        lanes = self.__dict__.get('_lane_list')
        if not lanes:
            return None
        cur = torch.cuda.current_stream(lanes[0]['ring'].device)
        for lane in lanes:
            if lane['dirty'] and lane['stream'] is not None:
                cur.wait_stream(lane['stream'])
        second = lanes[1]['grad'] if lanes[1]['dirty'] else None
        for lane in lanes:
            lane['dirty'] = False
        self.__dict__['_lane_next'] = 0
        return second

    def __getstate__(self):                          # lane streams / rings / graphs are run-time state, never pickled
        d = dict(self.__dict__)
        for k in ('_lane_list', '_lane_next', '_eval_acc'):
            d.pop(k, None)
        return d

    def check_device_status(self):
        """Raise MstError if a kernel reported a device-side failure (include/mst_amd.h MST_DEV_*: the multi-workgroup LSTM's
        exchange timing out) on any workspace used since the last check.  Synchronises; call it where the loop reads its
        losses back anyway (style.train.LossLog.flush does)."""
        self.join_lanes_keep()
        for plan in list(_native.get()._plans.values()):
            plan.check_touched()

    def join_lanes_keep(self):
        """Wait for the lanes without consuming their gradient bookkeeping (a health check is not an optimizer step)."""
        lanes = self.__dict__.get('_lane_list')
        if lanes:
            cur = torch.cuda.current_stream(lanes[0]['ring'].device)
            for lane in lanes:
                if lane['dirty'] and lane['stream'] is not None:
                    cur.wait_stream(lane['stream'])

    def forward(self, mode, bpm, pitched_channels, instruments_features, unpitched_channels=None):
        pitched_channels, unpitched_channels = self._dense(pitched_channels), self._dense(unpitched_channels)
        ip, mp, bp, xp, xu = _Forward.apply(self, self._anchor(), torch.is_grad_enabled(), mode, bpm, pitched_channels,
                                            instruments_features, unpitched_channels)
        return (ip, mp, bp), xp, (xu if unpitched_channels is not None else None)


def _scatter_records(roll, out, holder, dev):
    """Upload a SparseRoll's records and expand them into `out` (a lane's static note buffer), all enqueued on the current
    stream.  `holder` keeps, per feature count, the lane's device record buffer — grown by doubling, never per call — and the
    pinned staging slots for rolls whose records are not in pinned memory already."""
    if out is None or out.numel() != roll.n_cells * roll.nfeat:
        raise _native.MstError(f'{roll!r} does not have the shape of the note tensor it stands for')
    words = roll.packed.numel()
    slot = holder.setdefault(roll.nfeat, dict(dev=None, stage=[], at=0))
    if slot['dev'] is None or slot['dev'].numel() < words:
        grown = max(words, 2 * slot['dev'].numel() if slot['dev'] is not None else 1 << 12)
        slot['dev'] = torch.empty(grown, dtype=torch.int32, device=dev)       # (the old one is recycled in stream order)
    src = roll.packed
    if not src.is_pinned():
        # two staging slots, each reused only after the copy that last read it has completed: its event is waited for
        # (long over in the steady state: two calls of this lane have gone by)
        if not slot['stage']:
            slot['stage'] = [dict(buf=None, done=None) for _ in range(2)]
        stage = slot['stage'][slot['at'] % 2]
        slot['at'] += 1
        if stage['done'] is not None and not stage['done'].query():
            stage['done'].synchronize()
        if stage['buf'] is None or stage['buf'].numel() < words:
            stage['buf'] = torch.empty(max(words, 2 * stage['buf'].numel() if stage['buf'] is not None else 1 << 12),
                                       dtype=torch.int32, pin_memory=True)
        stage['buf'][:words].copy_(src)
        src = stage['buf'][:words]
        slot['dev'][:words].copy_(src, non_blocking=True)
        stage['done'] = stage['done'] or torch.cuda.Event()
        stage['done'].record()
    else:
        slot['dev'][:words].copy_(src, non_blocking=True)   # (the host allocator keeps a pinned block until this copy is over)
    scatter_packed(_native.get(), slot['dev'], roll.count, roll.n_cells, roll.nfeat, out, _native.current_stream(dev))


def _shapes(model, C, R, T):
    w = dict(_DEFAULT_WIDTHS)
    w.update(model._widths)
    return dict(style=(1, w['style']), melody=(1, R, T, 10, 56, w['melody']), rhythm=(1, R, T, 10, w['rhythm']),
                instruments_pred=(1, w['n_instruments']), mode_pred=(1, 2), bpm_pred=(1,),
                pitched_pred=(1, C, R, T, 10, 56, 5), unpitched_pred=(1, 1, R, T, 10, 47, 2))


def _seed(plan, ws, name, g):
    slot = plan.grad(name, ws=ws)
    if g is None:
        slot.zero_()
    else:
        slot.copy_(g.reshape(-1))


class _StageFn(torch.autograd.Function):
    """Common plumbing: one workspace per forward whose backward is pending (two grad-enabled forwards of the same
    shape may both be waiting for their backward, e.g. the summed loss of two clips); it comes from the plan's pool
    and goes back when that backward has run.  Without grad the plan's own scratch workspace is reused."""

    @staticmethod
    def _ws(plan, grad):
        return plan.acquire_ws() if grad else plan.ws

    @staticmethod
    def _take(ctx):
        """The saved state of a forward, exactly once: its workspace goes back to the pool after this backward."""
        stuff, ctx.stuff = ctx.stuff, None
        if stuff is None:
            raise _native.MstError('this stage was already back-propagated (its workspace has been recycled); '
                                   'run the forward again instead of retain_graph=True')
        return stuff


class _Extract(_StageFn):
    @staticmethod
    def forward(ctx, model, anchor, grad, mode, bpm, pitched, instr, unpitched):
        dev = anchor.device
        pitched = _f32c(pitched, dev)
        unpitched = None if unpitched is None else _f32c(unpitched, dev)
        _, C, R, T = pitched.shape[:4]
        plan = model._plan(C, R, T, unpitched is not None, dev)
        ws = _StageFn._ws(plan, grad)
        plan.set_inputs(mode=_f32c(mode, dev), bpm=_f32c(bpm, dev), instr=_f32c(instr, dev), ws=ws)
        plan.forward(_native.STAGE_EXTRACT, model._flat, pitched, unpitched, ws=ws)
        shp = _shapes(model, C, R, T)
        ctx.stuff = (model, plan, ws, pitched, unpitched)
        return tuple(plan.view(k, shp[k], ws=ws).clone() for k in ('style', 'melody', 'rhythm'))

    @staticmethod
    def backward(ctx, g_style, g_melody, g_rhythm):
        model, plan, ws, pitched, unpitched = _StageFn._take(ctx)
        plan.zero_grads(_native.STAGE_EXTRACT, ws=ws)
        for k, g in (('style', g_style), ('melody', g_melody), ('rhythm', g_rhythm)):
            _seed(plan, ws, k, g)
        plan.backward(_native.STAGE_EXTRACT, model._flat, model._grad_target(), pitched, unpitched, ws=ws)
        model._publish_grads()
        plan.release_ws(ws)
        return (None,) * 8


class _Predict(_StageFn):
    @staticmethod
    def forward(ctx, model, anchor, grad, style, rhythm):
        dev = anchor.device
        R, T = rhythm.shape[1:3]
        plan = model._plan(1, R, T, False, dev)
        ws = _StageFn._ws(plan, grad)
        plan.view('style', ws=ws).copy_(_f32c(style, dev).reshape(-1))
        plan.view('rhythm', ws=ws).copy_(_f32c(rhythm, dev).reshape(-1))
        plan.forward(_native.STAGE_INFO, model._flat, None, None, ws=ws)
        shp = _shapes(model, 1, R, T)
        ctx.stuff = (model, plan, ws)
        return tuple(plan.view(k, shp[k], ws=ws).clone() for k in ('instruments_pred', 'mode_pred', 'bpm_pred'))

    @staticmethod
    def backward(ctx, g_instr, g_mode, g_bpm):
        model, plan, ws = _StageFn._take(ctx)
        plan.zero_grads(_native.STAGE_INFO, ws=ws)
        for k in ('style', 'rhythm'):
            plan.grad(k, ws=ws).zero_()
        for k, g in (('instruments_pred', g_instr), ('mode_pred', g_mode), ('bpm_pred', g_bpm)):
            _seed(plan, ws, k, g)
        plan.backward(_native.STAGE_INFO, model._flat, model._grad_target(), None, None, ws=ws)
        model._publish_grads()
        shp = _shapes(model, 1, *[int(v) for v in (plan.dims.R, plan.dims.T)])
        out = (None, None, None, plan.grad('style', shp['style'], ws=ws).clone(), plan.grad('rhythm', shp['rhythm'], ws=ws).clone())
        plan.release_ws(ws)
        return out


class _Apply(_StageFn):
    @staticmethod
    def forward(ctx, model, anchor, grad, style, melody, rhythm, instr, unpitched):
        dev = anchor.device
        instr = _f32c(instr, dev)
        C = instr.shape[1]
        R, T = rhythm.shape[1:3]
        plan = model._plan(C, R, T, unpitched, dev)
        ws = _StageFn._ws(plan, grad)
        plan.set_inputs(instr=instr, ws=ws)
        for k, t in (('style', style), ('melody', melody), ('rhythm', rhythm)):
            plan.view(k, ws=ws).copy_(_f32c(t, dev).reshape(-1))
        plan.forward(_native.STAGE_APPLY, model._flat, None, None, ws=ws)
        shp = _shapes(model, C, R, T)
        ctx.stuff = (model, plan, ws, unpitched)
        xp = plan.view('pitched_pred', shp['pitched_pred'], ws=ws).clone()
        xu = plan.view('unpitched_pred', shp['unpitched_pred'], ws=ws).clone() if unpitched else xp.new_zeros(1)
        return xp, xu

    @staticmethod
    def backward(ctx, g_xp, g_xu):
        model, plan, ws, unpitched = _StageFn._take(ctx)
        plan.zero_grads(_native.STAGE_APPLY, ws=ws)
        for k in ('style', 'melody', 'rhythm'):
            plan.grad(k, ws=ws).zero_()
        _seed(plan, ws, 'pitched_pred', g_xp)
        if unpitched:
            _seed(plan, ws, 'unpitched_pred', g_xu)
        plan.backward(_native.STAGE_APPLY, model._flat, model._grad_target(), None, None, ws=ws)
        model._publish_grads()
        shp = _shapes(model, plan.dims.C, plan.dims.R, plan.dims.T)
        out = (None, None, None) + tuple(plan.grad(k, shp[k], ws=ws).clone() for k in ('style', 'melody', 'rhythm')) + (None, None)
        plan.release_ws(ws)
        return out


class _Forward(_StageFn):
    """extract_style + predict_song_info + apply_style in one workspace (the training path)."""

    @staticmethod
    def forward(ctx, model, anchor, grad, mode, bpm, pitched, instr, unpitched):
        dev = anchor.device
        pitched = _f32c(pitched, dev)
        unpitched = None if unpitched is None else _f32c(unpitched, dev)
        _, C, R, T = pitched.shape[:4]
        U = unpitched is not None
        plan = model._plan(C, R, T, U, dev)
        ws = _StageFn._ws(plan, grad)
        plan.set_inputs(mode=_f32c(mode, dev), bpm=_f32c(bpm, dev), instr=_f32c(instr, dev), ws=ws)
        plan.forward(_native.STAGE_ALL, model._flat, pitched, unpitched, ws=ws)
        shp = _shapes(model, C, R, T)
        ctx.stuff = (model, plan, ws, pitched, unpitched)
        keys = ['instruments_pred', 'mode_pred', 'bpm_pred', 'pitched_pred']
        outs = [plan.view(k, shp[k], ws=ws).clone() for k in keys]
        outs.append(plan.view('unpitched_pred', shp['unpitched_pred'], ws=ws).clone() if U else outs[0].new_zeros(1))
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_instr, g_mode, g_bpm, g_xp, g_xu):
        model, plan, ws, pitched, unpitched = _StageFn._take(ctx)
        plan.zero_grads(_native.STAGE_ALL, ws=ws)
        for k, g in (('instruments_pred', g_instr), ('mode_pred', g_mode), ('bpm_pred', g_bpm), ('pitched_pred', g_xp)):
            _seed(plan, ws, k, g)
        if unpitched is not None:
            _seed(plan, ws, 'unpitched_pred', g_xu)
        plan.backward(_native.STAGE_ALL, model._flat, model._grad_target(), pitched, unpitched, ws=ws)
        model._publish_grads()
        plan.release_ws(ws)
        return (None,) * 8


# ---- losses (style/model.py:847-997) --------------------------------------------------------
class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pp, pt, up, ut, il, it, ml, mt, bp, bt, normalize):
        lib = _native.get().lib
        dev = pp.device
        if dev.type != 'cuda':
            raise _native.MstError('get_total_loss needs GPU tensors; there is no CPU fallback')
        pp, pt, il, it, ml, mt, bp, bt = (_f32c(t, dev) for t in (pp, pt, il, it, ml, mt, bp, bt))
        has_u = up is not None and ut is not None
        up, ut = (_f32c(up, dev), _f32c(ut, dev)) if has_u else (None, None)
        losses = torch.empty(_native.N_LOSSES, dtype=torch.float32, device=dev)
        saved = torch.empty(_native.LOSS_SAVED, dtype=torch.float32, device=dev)
        scratch = torch.empty(lib.mst_loss_scratch_floats(), dtype=torch.float32, device=dev)
        n_p = pp.numel() // 5
        n_u = up.numel() // 2 if has_u else 0
        P = _native.ptr
        _native.check(lib.mst_total_loss_fwd(P(pp), P(pt), n_p, P(up), P(ut), n_u, P(il), P(it), il.numel(), P(ml), P(mt),
                                             P(bp), P(bt), int(normalize), P(losses), P(saved), P(scratch),
                                             _native.current_stream(dev)), 'mst_total_loss_fwd')
        ctx.stuff = (pp, pt, up, ut, il, it, ml, mt, bp, bt, saved, n_p, n_u)
        return losses

    @staticmethod
    def backward(ctx, gl):
        pp, pt, up, ut, il, it, ml, mt, bp, bt, saved, n_p, n_u = ctx.stuff
        lib = _native.get().lib
        dev = pp.device
        gl = torch.nan_to_num(_f32c(gl, dev))
        g_pp, g_il, g_ml, g_bp = (torch.empty_like(t) for t in (pp, il, ml, bp))
        g_up = torch.empty_like(up) if up is not None else None
        P = _native.ptr
        _native.check(lib.mst_total_loss_bwd(P(pp), P(pt), n_p, P(up), P(ut), n_u, P(il), P(it), il.numel(), P(ml), P(mt),
                                             P(bp), P(bt), P(saved), P(gl), P(g_pp), P(g_up), P(g_il), P(g_ml), P(g_bp),
                                             _native.current_stream(dev)), 'mst_total_loss_bwd')
        return g_pp, None, g_up, None, g_il, None, g_ml, None, g_bp, None, None


class LossDict(dict):
    """The reference's nested loss dict; `.packed` is the 15-leaf device tensor behind it (key order
    `_native.LOSS_KEYS`, NaN for absent unpitched leaves) so a training loop can log without a sync per leaf."""

    def __init__(self, packed, **items):
        super().__init__(**items)
        self.packed = packed


def get_total_loss(instruments_pred, instruments_target, mode_pred, mode_target, bpm_pred, bpm_target,
                   pitched_pred, pitched_target, unpitched_pred=None, unpitched_target=None, normalize=False):
    """Same nested dict as the reference (style/model.py:944-996).  Positional contract preserved: the
    third/fourth slots are consumed as (bpm prediction, bpm target) and the fifth/sixth as (mode logits,
    one-hot mode) — the reference's pack/unpack swap at :900-901 vs :976-977, which is how
    train-model.py:115-122 calls it (bpm before mode)."""
    dev = pitched_pred.device
    bpm_p, bpm_t, mode_p, mode_t = mode_pred, mode_target, bpm_pred, bpm_target
    bpm_t = torch.as_tensor(bpm_t, dtype=torch.float32, device=dev).reshape(-1)[:1]
    L = _Loss.apply(pitched_pred, pitched_target, unpitched_pred if unpitched_target is not None else None,
                    unpitched_target, instruments_pred, instruments_target, mode_p, mode_t, bpm_p.reshape(-1), bpm_t,
                    bool(normalize))
    k = {name: i for i, name in enumerate(_native.LOSS_KEYS)}
    pitched = dict(total=L[k['channels_loss_pitched_total']], notes_loss=L[k['channels_loss_pitched_notes_loss']],
                   velocity_loss=L[k['channels_loss_pitched_velocity_loss']],
                   duration_loss=L[k['channels_loss_pitched_duration_loss']],
                   accidentals_loss=L[k['channels_loss_pitched_accidentals_loss']])
    unpitched = None
    if unpitched_target is not None:
        unpitched = dict(total=L[k['channels_loss_unpitched_total']], notes_loss=L[k['channels_loss_unpitched_notes_loss']],
                         velocity_loss=L[k['channels_loss_unpitched_velocity_loss']],
                         duration_loss=L[k['channels_loss_unpitched_duration_loss']])
    one = lambda name: L[k[name]:k[name] + 1]      # shape (1,), like the reference's bpm-derived leaves
    return LossDict(L.detach(),
        total=one('total'),
        channels_loss=dict(total=L[k['channels_loss_total']], pitched=pitched, unpitched=unpitched),
        song_info_loss=dict(total=one('song_info_loss_total'), instruments_loss=L[k['song_info_loss_instruments_loss']],
                            mode_loss=L[k['song_info_loss_mode_loss']], bpm_loss=one('song_info_loss_bpm_loss')),
    )


def hard_output(x):
    """style/model.py:818-832 — like the reference it also zeroes sub-threshold velocities of `x` in place."""
    if x.device.type != 'cuda':
        raise _native.MstError('hard_output needs a GPU tensor; there is no CPU fallback')
    nfeat = x.shape[-1]
    work = x if (x.is_contiguous() and x.dtype == torch.float32) else x.detach().float().contiguous()
    out = torch.empty_like(work)
    _native.check(_native.get().lib.mst_hard_output(_native.ptr(work.detach()), _native.ptr(out), work.numel() // nfeat, nfeat,
                                                    _native.current_stream(x.device)), 'mst_hard_output')
    if work is not x:
        with torch.no_grad():
            x[..., 1] = work[..., 1].to(x.dtype)
    return out


def hard_output_sparse(x):
    """`hard_output` (style/model.py:818-832) as sorted note records: a host `style.data.SparseRoll` of the cells whose hard
    velocity is non-zero, with their hard features — what the MIDI decoder reads of the dense result.  The records are built on
    the GPU (mst_roll_count / mst_roll_compact) and only they are downloaded.  Unlike `hard_output` it leaves `x` untouched."""
    if x.device.type != 'cuda':
        raise _native.MstError('hard_output_sparse needs a GPU tensor; there is no CPU fallback')
    return compact(x, 'hard')
