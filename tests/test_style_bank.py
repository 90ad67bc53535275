"""The style bank on the CPU: mst_style_put, mst_style_mix and mst_info_decide (the product's kernel source on the hipsim
interpreter, the cases of tests/style_bank_cases.py), their chain with the crops, mst_window_inputs and the stage masks of
mst_forward at the C ABI, and the host side of style.data.StyleBank."""
import numpy as np
import pytest
import torch

import simutil
import style_bank_cases as sb


@pytest.mark.parametrize('case', sb.KERNEL_CASES, ids=[c.__name__[5:] for c in sb.KERNEL_CASES])
def test_kernels(case):
    case(simutil.sim_native(), 'cpu')


def test_chain_at_the_c_abi():
    sb.case_chain(simutil.sim_native(), 'cpu', K=3)


# ---- the host side
def filled_bank(capacity=1):
    from style.data import StyleBank
    bank = StyleBank(5, 'cpu', capacity=capacity)
    rng = np.random.default_rng(2)
    words = rng.integers(0, 2 ** 32, (6, 5), dtype=np.uint64).astype(np.uint32)
    words[0, :4] = (0x7fa00001, 0xffc12345, 0x80000000, 0x00000001)             # NaN payloads, -0.0 and a denormal are kept
    names = ['first', 'first', 7, 'second', 7, 'first']
    for k, name in enumerate(names):
        assert bank.add(name, 2 * k, 2, torch.from_numpy(words[k].view(np.float32))) == k
    return bank, words, names


def test_style_bank_entries_blends_and_csr():
    """song() is the mean with float32 weights, blend() scales and concatenates, mix() is the CSR mst_style_mix reads; the bank
    grows by doubling and keeps its rows."""
    from style.data import StyleBank
    bank, words, names = filled_bank()
    assert len(bank) == 6 and bank.capacity == 8 and np.array_equal(sb.words(bank.rows[:6]).reshape(6, 5), words)
    assert (bank.rows[6:] == 0).all() and bank.by_song == {'first': [0, 1, 5], 7: [2, 4], 'second': [3]}
    assert bank.provenance == [(n, 2 * k, 2) for k, n in enumerate(names)]
    third = np.float32(1.) / np.float32(3.)
    assert bank.song('first') == [(0, third), (1, third), (5, third)] and bank.row(4) == [(4, np.float32(1.))]
    assert all(isinstance(w, np.float32) for _, w in bank.song('first'))
    blend = bank.blend([('first', .3), (bank.row(4), .5), (7, -.2), (bank.blend([('second', .5)]), .5)])
    assert [r for r, _ in blend] == [0, 1, 5, 4, 2, 4, 3]
    half = np.float32(.5)
    want = [third * np.float32(.3)] * 3 + [half, half * np.float32(-.2), half * np.float32(-.2), half * half]
    assert [w for _, w in blend] == want and all(isinstance(w, np.float32) for _, w in blend)
    offsets, idx, w = StyleBank.mix([bank.row(1), blend, bank.song(7)])
    assert offsets.dtype == idx.dtype == np.int32 and w.dtype == np.float32
    assert offsets.tolist() == [0, 1, 8, 10] and idx.tolist() == [1, 0, 1, 5, 4, 2, 4, 3, 2, 4] and w.tolist() == [1.] + want + [.5, .5]
    assert StyleBank.mix([[], bank.row(0)])[0].tolist() == [0, 0, 1]
    for bad in (lambda: bank.song('third'), lambda: bank.row(6), lambda: bank.row(-1)):
        with pytest.raises(KeyError):
            bad()
    for bad in (lambda: bank.blend([]), lambda: bank.add('x', 0, 2, torch.zeros(4)), lambda: StyleBank(0, 'cpu')):
        with pytest.raises(ValueError):
            bad()


def test_style_bank_save_and_load_round_trip(tmp_path):
    """The rows' bits and the provenance — names that are strings and names that are ints — survive save / load."""
    from style.data import StyleBank
    bank, words, names = filled_bank(capacity=3)
    path = tmp_path / 'library.npz'
    bank.save(str(path))
    back = StyleBank.load(str(path), 'cpu')
    assert len(back) == 6 and back.style_size == 5 and np.array_equal(sb.words(back.rows[:6]).reshape(6, 5), words)
    assert back.provenance == bank.provenance and back.by_song == bank.by_song and 7 in back.by_song and '7' not in back.by_song
    assert back.song('first') == bank.song('first')
    assert back.add('later', 0, 2, torch.ones(5)) == 6 and back.capacity >= 7             # a loaded bank goes on growing
    assert np.array_equal(sb.words(back.rows[:6]).reshape(6, 5), words)
    empty = StyleBank(5, 'cpu')
    empty.save(str(path))
    assert len(StyleBank.load(str(path), 'cpu')) == 0
