"""-m gpu: the sparse output path on an MI355X.  mst_roll_count / mst_roll_compact must give the records of the dense path bit
for bit — `sparsify` in nonzero mode, the oracle's hard_output in hard mode — eagerly and replayed from a captured graph, and
the inference driver must write the same bytes with sparse_output=True as without."""
import os

import numpy as np
import pytest
import torch

from tools.synth import synth_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HERE = os.path.dirname(os.path.abspath(__file__))
MIDI = os.path.join(HERE, 'golden', 'midi')
NAN = float('nan')


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_records(roll, cells, feats, shape):
    return roll.shape == tuple(shape) and roll.count == len(cells) and torch.equal(roll.cells, cells) and \
        feats.shape == roll.feats.shape and torch.equal(_bits(roll.feats), _bits(feats))


def _want_hard(x):
    """Records of the oracle's dense hard roll: the cells with a non-zero velocity, with the hard features."""
    from oracle import style_oracle as so
    flat = so.hard_output(x.clone()).view(-1, x.shape[-1])
    idx = torch.from_numpy(np.flatnonzero(flat[:, 1].numpy()))
    return idx.to(torch.int32), flat[idx]


def _near_threshold(x, seed):
    """A third of the live velocities scaled to around the .01 threshold, so that hard mode is not nonzero mode."""
    g = torch.Generator().manual_seed(seed)
    x = x.clone()
    quiet = torch.rand(x.shape[:-1], generator=g) < .3
    x[..., 1] = torch.where(quiet, x[..., 1] * .02, x[..., 1])
    return x


_CLIPS = {}


def _clip(crt):
    if crt not in _CLIPS:
        clip = synth_clip(1, *crt, True)
        _CLIPS[crt] = [_near_threshold(clip[k], 5 + i) for i, k in enumerate(('pitched', 'unpitched'))]
    return _CLIPS[crt]


@pytest.mark.parametrize('crt', [(4, 16, 4), (8, 151, 4)])
def test_compact_is_bit_equal(crt):
    from style import _native
    from style.data import compact, sparsify
    for x in _clip(crt):
        n_cells = x.numel() // x.shape[-1]
        assert n_cells in (143360, 30080, 2705920, 283880)         # 143360 is whole slices, the others end in a ragged one
        if crt[1] == 151 and x.shape[-1] == 5:
            assert _native.get().roll_slices(n_cells) > 2048     # more slices than one pass of the scan workgroup covers
        xd = x.to(DEV)
        want = sparsify(x)
        got = compact(xd, 'nonzero')
        assert got.packed.is_pinned() and _same_records(got, want.cells, want.feats, x.shape)
        cells, feats = _want_hard(x)
        assert 0 < len(cells) < want.count
        assert _same_records(compact(xd, 'hard'), cells, feats, x.shape)
        assert torch.equal(_bits(xd.cpu()), _bits(x))            # the source is read only


def test_compact_at_full_density():
    from style.data import compact, sparsify
    x = synth_clip(1, 4, 16, 4, True, density=1.)['pitched']
    want = sparsify(x)
    assert want.count == want.n_cells == 143360
    xd = x.to(DEV)
    assert _same_records(compact(xd, 'nonzero'), want.cells, want.feats, x.shape)
    cells, feats = _want_hard(x)
    assert len(cells) == 143360
    assert _same_records(compact(xd, 'hard'), cells, feats, x.shape)


def test_hard_output_sparse_leaves_its_input_alone():
    from style.model import hard_output, hard_output_sparse
    x = _clip((4, 16, 4))[0]
    xd = x.to(DEV)
    roll = hard_output_sparse(xd)
    assert torch.equal(_bits(xd.cpu()), _bits(x))
    work = xd.clone()
    dense = hard_output(work).cpu().view(-1, 5)
    assert not torch.equal(work.cpu(), x)                        # hard_output did zero velocities of ITS input
    idx = torch.from_numpy(np.flatnonzero(dense[:, 1].numpy()))
    assert _same_records(roll, idx.to(torch.int32), dense[idx], x.shape)
    with pytest.raises(Exception, match='GPU tensor'):
        hard_output_sparse(x)


def test_count_and_compact_replay_from_a_captured_graph():
    from style import _native
    from style.data import compact
    native = _native.get()
    first, second = _clip((4, 16, 4))[0], _near_threshold(synth_clip(2, 4, 16, 4, True)['pitched'], 9)
    n_cells, capacity = first.numel() // 5, 4096
    static = first.to(DEV)
    ws = torch.zeros(native.roll_slices(n_cells) + 1, dtype=torch.int32, device=DEV)
    cells = torch.full((capacity,), -7, dtype=torch.int32, device=DEV)
    feats = torch.full((capacity, 5), NAN, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # a single chain on the capture stream
        stream = _native.current_stream(DEV)
        native.roll_count(static, n_cells, 5, _native.ROLL_HARD, ws, stream)
        native.roll_compact(static, n_cells, 5, _native.ROLL_HARD, ws, capacity, cells, feats, stream)
    for x in (first, second):
        static.copy_(x)
        cells.fill_(-7)
        feats.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        want = compact(x.to(DEV), 'hard')                        # the eager result
        n = int(ws[-1])
        assert 0 < n == want.count < capacity
        assert torch.equal(cells[:n].cpu(), want.cells) and torch.equal(_bits(feats[:n].cpu()), _bits(want.feats))
        assert (cells[n:] == -7).all() and torch.isnan(feats[n:]).all()
    assert not torch.equal(_bits(first), _bits(second))


def test_save_writes_the_same_file_from_records(tmp_path):
    from style import style_transfer as st
    from style.midi_conversion import ChannelConverter
    _, (info, _, _, instruments, _) = st.get_model_input(os.path.join(MIDI, 'Dancing in the Moonlight.mid'))
    assert len(instruments) >= 3
    g = torch.Generator().manual_seed(3)
    clip = synth_clip(7, 3, 5, 4, True, density=.035)
    pitched, unpitched = _near_threshold(clip['pitched'], 1), _near_threshold(clip['unpitched'], 2)
    pitched[..., 2:] = torch.rand(pitched.shape[:-1] + (3,), generator=g) * (pitched[..., 1:2] != 0)     # soft accidentals
    assert tuple(pitched.shape) == (1, 3, 5, 4, 10, 56, 5) and tuple(unpitched.shape) == (1, 1, 5, 4, 10, 47, 2)
    assert .02 < float((pitched[..., 1] > .01).float().mean()) < .04
    files = {}
    for sparse_output in (False, True):
        path = str(tmp_path / f'{int(sparse_output)}' / 'song.mid')
        st.save(ChannelConverter(info), pitched.to(DEV), unpitched.to(DEV), instruments[:3], path, sparse_output=sparse_output)
        files[sparse_output] = open(path, 'rb').read()
    assert len(files[False]) > 2000 and files[True] == files[False]


def test_transfer_style_writes_the_same_files_from_records(tmp_path):
    """The one longer test: the end-to-end driver twice (the slow step of both runs is the host decode)."""
    from style import style_transfer as st
    from style.data import percussion_id
    from test_host_surface import FULL, build_model
    from test_style_transfer import DRUMS_COMPOSITION, DRUMS_STYLE
    model = build_model(FULL, seed=108).to(DEV)
    with torch.no_grad():                                        # as in test_style_transfer: have the model pick percussion
        model.song_info_model.instruments_linear.bias[percussion_id] += 10.
    written = {}
    for sparse_output in (False, True):
        out = str(tmp_path / f'{int(sparse_output)}')
        st.transfer_style(model, DRUMS_COMPOSITION, [DRUMS_STYLE], out, sparse_output=sparse_output)
        written[sparse_output] = {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), 'rb').read()
                                  for d, _, names in os.walk(out) for f in names if f.endswith('.mid')}
    assert len(written[False]) == 4 and all(len(b) > 1000 for b in written[False].values())
    assert sorted(written[True]) == sorted(written[False])
    for name, data in written[False].items():
        assert written[True][name] == data, name
