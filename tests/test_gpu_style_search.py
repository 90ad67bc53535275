"""-m gpu: style search on an MI355X.  mst_style_search (the cases of tests/style_search_cases.py: the bound against float64,
the constructed order and position independence — the bit comparison with the host chain is tools/window_rate.py --search's to
report), StyleTransferModel.transfer_styles with mix=Nearest(k) against the same call with the explicit CSR, and
style_transfer.transfer_songs with a library."""
import os

import numpy as np
import pytest
import torch

import eval_cases as ec
import eval_window_cases as wc
import style_search_cases as sc
import transfer_cases as tc
from test_gpu_eval_windows import batches, small_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C, T, BARS = wc.C, wc.T, wc.BARS


def _native():
    from style import _native
    return _native.get()


@pytest.mark.parametrize('case', sc.KERNEL_CASES, ids=[c.__name__[5:] for c in sc.KERNEL_CASES])
def test_kernels(case):
    case(_native(), DEV)
    torch.cuda.synchronize()


# ---- transfer_styles(mix=Nearest(k))
def bank_of_every_window(model, store, K):
    """Every window of every song (stride 1), encoded K at a time — the tiling of the plan that renders, so that a window's row
    is the bits of its own style there —, and {(song, first bar): row}."""
    bank = model.encode_styles(store, BARS, K, stride=1)
    torch.cuda.synchronize()
    return bank, {(song, r0): row for row, (song, r0, bars) in enumerate(bank.provenance)}


def same_render(got, want, K):
    for name in ('instruments_pred', 'mode_pred', 'bpm_pred', 'instr_features', 'decisions'):
        a, b = getattr(got, name), getattr(want, name)
        assert ec.same_bits(a, b) if a.dtype != torch.int32 else torch.equal(a, b), name
        assert a.dtype == torch.int32 or torch.isfinite(a).all(), name
    for k in range(K):
        for mine, ref in ((got.pitched[k], want.pitched[k]), (got.unpitched[k], want.unpitched[k])):
            assert mine.count == ref.count and torch.equal(mine.packed, ref.packed), k
        assert 0 < got.pitched[k].count < got.pitched[k].n_cells


def nearest_states(plan):
    return [key for st in plan.__dict__['_transfer_style_state'].values() for key in st['graphs']
            if any(isinstance(x, tuple) and x and x[0] == 'nearest' for x in key)]


def test_transfer_styles_nearest_is_the_explicit_mix_of_the_neighbours():
    """encode_styles, then transfer_styles(mix=Nearest(3)) on three batches — eager, captured, replayed, the bank growing between
    the second and the third: the neighbours never name a row of the clip's own song, pass the validity check of the kernel cases
    against the bank's rows with the clips' own styles as queries, and everything rendered equals, bit for bit, a second call
    with the explicit CSR of those rows and the weights float32(1) / float32(3).  One graph serves the second and third use."""
    from style.data import Nearest
    K, k = 3, 3
    model = small_model()
    store = wc.make_store(DEV)
    bank, row_of = bank_of_every_window(model, store, K)
    plan = model._plan(C, BARS, T, True, torch.device(DEV), clips=K)
    plan.__dict__.pop('_transfer_style_state', None)
    third = np.float32(1.) / np.float32(3.)
    grown = False
    for n, batch in enumerate(batches(K)):
        if n == 2:                                              # the bank grows (inside its capacity): a near copy of every row
            before, address = len(bank), bank.rows.data_ptr()
            for r in range(before):
                bank.add('elsewhere', r, BARS, bank.rows[r] * 1.0009765625)
            grown = True
            assert len(bank) == 2 * before and bank.rows.data_ptr() == address
        got = model.transfer_styles(store, batch, bank, Nearest(k))
        torch.cuda.synchronize()
        songs, r0s = batch.songs.tolist(), batch.r0s.tolist()
        rows, scores = got.neighbours.cpu().numpy(), got.neighbour_scores.cpu().numpy()
        assert rows.shape == scores.shape == (K, k) and rows.dtype == np.int32 and scores.dtype == np.float32
        for q in range(K):
            assert all(bank.provenance[r][0] != songs[q] for r in rows[q])
        queries = bank.rows[[row_of[s, r0] for s, r0 in zip(songs, r0s)]].cpu().numpy()
        sc.check_ranking(rows, scores.view(np.uint32), queries, bank.rows[:len(bank)].cpu().numpy(), k, 1,
                         groups=bank.device_groups()[:len(bank)].tolist(), exclude=[bank.group_of(s) for s in songs])
        if grown:
            assert (rows >= before).any()                       # the replay saw the rows added since the capture
        explicit = (np.arange(K + 1) * k, rows.reshape(-1), np.full(K * k, third, dtype=np.float32))
        want = model.transfer_styles(store, batch, bank, explicit)
        torch.cuda.synchronize()
        same_render(got, want, K)
        assert want.neighbours is None and want.neighbour_scores is None
        assert len(nearest_states(plan)) == (1 if n >= 1 else 0), (n, nearest_states(plan))
    model.check_device_status()


def test_nearest_without_exclusion_finds_the_clips_own_window_and_scores():
    """exclude_own=False: every clip's first neighbour is its own window's row, or a bit-identical duplicate of it; farthest
    first passes the same validity check; score=True works as before, against the blend of the neighbours; too few foreign
    rows is a ValueError on the host."""
    from style.data import Nearest
    K = 3
    model = small_model()
    store = wc.make_store(DEV)
    bank, row_of = bank_of_every_window(model, store, K)
    batch = batches(K)[1]
    songs, r0s = batch.songs.tolist(), batch.r0s.tolist()
    own = [row_of[s, r0] for s, r0 in zip(songs, r0s)]
    all_rows = bank.rows[:len(bank)].cpu().numpy()
    got = model.transfer_styles(store, batch, bank, Nearest(2, exclude_own=False), score=True)
    torch.cuda.synchronize()
    rows = got.neighbours.cpu().numpy()
    for q in range(K):
        assert np.array_equal(all_rows[rows[q, 0]].view(np.uint32), all_rows[own[q]].view(np.uint32)), (q, rows[q], own[q])
    sc.check_ranking(rows, got.neighbour_scores.cpu().numpy().view(np.uint32), all_rows[own], all_rows, 2, 1)
    assert torch.isfinite(got.style_sums).all() and np.isfinite(got.cosines).all()
    far = model.transfer_styles(store, batch, bank, Nearest(2, farthest=True))
    torch.cuda.synchronize()
    sc.check_ranking(far.neighbours.cpu().numpy(), far.neighbour_scores.cpu().numpy().view(np.uint32), all_rows[own], all_rows, 2, -1,
                     groups=bank.device_groups()[:len(bank)].tolist(), exclude=[bank.group_of(s) for s in songs])
    with pytest.raises(ValueError, match='fewer than'):
        model.transfer_styles(store, batch, bank, Nearest(16))
    model.check_device_status()


def test_nearest_leaves_the_training_state_alone():
    """Parameters and Adam moments hold the same bits before and after encode_styles and transfer_styles(mix=Nearest)."""
    from style.data import Nearest
    from style.optim import FusedAdam
    K = 3
    store = wc.make_store(DEV)
    model = small_model()
    opt = FusedAdam(model)
    opt.zero_grad()
    model.train_windows(store, batches(K)[0])
    opt.step()
    torch.cuda.synchronize()
    before = [t.clone() for t in (model._flat, model._gflat, opt.exp_avg, opt.exp_avg_sq, opt.state)]
    bank = model.encode_styles(store, BARS, K)
    for batch in batches(K):
        got = model.transfer_styles(store, batch, bank, Nearest(2))
    torch.cuda.synchronize()
    assert (got.neighbours >= 0).all()
    for now, was in zip((model._flat, model._gflat, opt.exp_avg, opt.exp_avg_sq, opt.state), before):
        assert ec.same_bits(now, was)
    model.check_device_status()


# ---- the driver
def test_transfer_songs_with_a_library(tmp_path):
    """transfer_songs(library=, nearest=2) writes '{composition} (library style).mid' beside the files of the defaults, which
    are byte for byte those of a run made before; the provenance it returns per window is bank.search's, driven from the host
    with the windows' own styles; a library given as a path is loaded."""
    from style import style_transfer as st
    from style.data import SongStore, StyleBank, included_instruments as programs, prepare_input_sparse
    K, bars = 3, 2
    model = small_model()
    composition = tc.write_song(tmp_path / 'tune.mid', 1, 3, programs[:2])
    first = tc.write_song(tmp_path / 'first.mid', 2, 4, programs[2:4], bpm=140)
    second = tc.write_song(tmp_path / 'second.mid', 3, 4, programs[1:3], bpm=80)
    assert st.transfer_songs(model, composition, [first], str(tmp_path / 'plain'), bars=bars, K=K) is None
    plain = {name: (tmp_path / 'plain' / 'tune' / name).read_bytes() for name in os.listdir(tmp_path / 'plain' / 'tune')}
    # the library: every sounding window of the two style songs, under their names
    store = SongStore(DEV)
    for path in (first, second):
        store.add(prepare_input_sparse(st.get_model_input(path)))
    encoded = model.encode_styles(store, bars, K, stride=1)
    library = StyleBank(encoded.style_size, DEV)
    for row, (song, r0, n) in enumerate(encoded.provenance):
        library.add(('first', 'second')[song], r0, n, encoded.rows[row])
    assert len(library) >= 4 and len(library.by_song) == 2
    saved = tmp_path / 'library.npz'
    library.save(str(saved))
    out = st.transfer_songs(model, composition, [first], str(tmp_path / 'with'), bars=bars, K=K, library=library, nearest=2)
    torch.cuda.synchronize()
    files = {name: (tmp_path / 'with' / 'tune' / name).read_bytes() for name in os.listdir(tmp_path / 'with' / 'tune')}
    assert sorted(files) == sorted(list(plain) + ['tune (library style).mid']) and len(files['tune (library style).mid']) > 200
    assert all(files[name] == plain[name] for name in plain)
    assert set(out) == {'library'}
    # the composition's full, sounding windows encoded in the renderer's tiling are the queries
    alone = SongStore(DEV)
    alone.add(prepare_input_sparse(st.get_model_input(composition)))
    own = model.encode_styles(alone, bars, K)
    assert len(own) >= 1 and len(out['library']) >= len(own)
    rows, _ = library.search(own.rows[:len(own)], 2)
    for (_, r0, _), picked in zip(own.provenance, rows.tolist()):
        assert out['library'][r0 // bars] == [library.provenance[r] for r in picked]
    assert all(len(window) == 2 and all(name in ('first', 'second') for name, _, _ in window) for window in out['library'])
    again = st.transfer_songs(model, composition, [], str(tmp_path / 'path'), bars=bars, K=K, library=str(saved), nearest=2, score=True)
    assert again['library'] == out['library'] and np.isfinite(again['library style']['cosines']).all()
    assert (tmp_path / 'path' / 'tune' / 'tune (library style).mid').read_bytes() == files['tune (library style).mid']
    st.transfer_songs(model, composition, [first], str(tmp_path / 'after'), bars=bars, K=K)
    assert {name: (tmp_path / 'after' / 'tune' / name).read_bytes() for name in os.listdir(tmp_path / 'after' / 'tune')} == plain
    with pytest.raises(ValueError):
        st.transfer_songs(model, composition, [first], str(tmp_path / 'bad'), bars=bars, K=K, nearest=2)
    model.check_device_status()
