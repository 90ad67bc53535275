"""Style search on the CPU: mst_style_search (the product's kernel source on the hipsim interpreter, the cases of
tests/style_search_cases.py — there every score must equal the float32 fmaf chain of the header bit for bit and the rows its
ranking, ties included) and the host side of style.data.StyleBank: groups, search, song_means, neighbours, Nearest."""
import numpy as np
import pytest
import torch

import simutil
import style_bank_cases as sb
import style_search_cases as sc


@pytest.mark.parametrize('case', sc.KERNEL_CASES, ids=[c.__name__[5:] for c in sc.KERNEL_CASES])
def test_kernels(case):
    case(simutil.sim_native(), 'cpu', exact=True)


# ---- the host side
NAMES = ['first', 'first', 7, 'second', 7, 'first', 'third', 'second']
SIZE = 6


def filled_bank(capacity=1):
    from style.data import StyleBank
    bank = StyleBank(SIZE, 'cpu', capacity=capacity)
    rows = sc.values(len(NAMES), SIZE, seed=3)
    for k, name in enumerate(NAMES):
        assert bank.add(name, 2 * k, 2 + k % 2, torch.from_numpy(rows[k])) == k
    return bank, rows


def groups_of(bank):
    return bank.device_groups()[:len(bank)].tolist()


def test_groups_follow_the_songs_through_add_take_growth_save_and_load(tmp_path):
    """A row's group is the ordinal of its song in by_song's insertion order; the device copy is sized with the rows, refreshed
    at the next use and -1 behind the rows taken; save / load need no field for it."""
    from style.data import StyleBank
    bank, _ = filled_bank()
    want = [0, 0, 1, 2, 1, 0, 3, 2]
    assert list(bank.by_song) == ['first', 7, 'second', 'third'] and bank.capacity == 8
    assert groups_of(bank) == want and bank.groups.dtype == torch.int32 and len(bank.groups) == bank.capacity
    assert [bank.group_of(s) for s in ('first', 7, 'second', 'third')] == [0, 1, 2, 3]
    assert bank.group_of('7') == -1 and bank.group_of('fourth') == -1 and bank.group_of(None) == -1
    assert bank.take('fourth', 0, 2) == 8 and bank.capacity == 16 and bank.take(7, 4, 2) == 9          # it grew: the copy is rebuilt
    assert len(bank.groups) == 16 and groups_of(bank) == want + [4, 1] and (bank.groups[10:] == -1).all()
    assert bank.add('first', 9, 2, torch.ones(SIZE)) == 10 and groups_of(bank) == want + [4, 1, 0]
    path = tmp_path / 'library.npz'
    bank.save(str(path))
    back = StyleBank.load(str(path), 'cpu')
    assert groups_of(back) == groups_of(bank) and [back.group_of(s) for s in back.by_song] == [0, 1, 2, 3, 4]
    assert back.add('sixth', 0, 2, torch.ones(SIZE)) == 11 and groups_of(back)[-1] == 5
    assert StyleBank(SIZE, 'cpu').device_groups().tolist() == [-1] * 64


def test_search_with_tensor_and_entry_list_queries():
    """bank.search against the float32 chain in numpy: tensor queries, entry lists (mixed by mst_style_mix first), an excluded
    song per query, the farthest, k above the rows left; only the first len(bank) rows are searched."""
    native = simutil.sim_native()
    bank, rows = filled_bank(capacity=32)
    bank.rows[len(bank):] = torch.from_numpy(rows[:1])              # what lies behind the rows taken is never a neighbour
    queries = sc.values(3, SIZE, seed=4)
    everyone = np.ones(len(NAMES), dtype=bool)
    for farthest in (False, True):
        order = -1 if farthest else 1
        got_rows, got_scores = bank.search(torch.from_numpy(queries), 3, farthest=farthest, native=native)
        assert got_rows.shape == got_scores.shape == (3, 3) and got_rows.dtype == np.int32 and got_scores.dtype == np.float32
        c32 = sc.chain(queries, rows)
        for q in range(3):
            want = sc.ranking(c32[q], everyone, 3, order)
            assert got_rows[q].tolist() == want and np.array_equal(got_scores[q].view(np.uint32), c32[q, want].view(np.uint32))
    entries = [bank.row(4), bank.song('first'), bank.blend([('second', .25), (7, -1.5)])]
    offsets, idx, w = bank.mix(entries)
    mixed = np.stack([sb.mixed(rows.reshape(-1), len(NAMES), SIZE, offsets, idx, w, q, SIZE).view(np.float32) for q in range(3)])
    exclude = [7, None, 'nowhere']
    got_rows, got_scores = bank.search(entries, 8, exclude=exclude, native=native)
    c32 = sc.chain(mixed, rows)
    for q in range(3):
        rankable = np.asarray([name != exclude[q] for name in NAMES])
        want = sc.ranking(c32[q], rankable, 8, 1)
        assert got_rows[q].tolist() == want and (q == 0) == (-1 in want)
        live = [r for r in want if r >= 0]
        assert np.array_equal(got_scores[q, :len(live)].view(np.uint32), c32[q, live].view(np.uint32)) and np.isnan(got_scores[q, len(live):]).all()
    assert 4 not in got_rows[0] and 2 not in got_rows[0] and got_rows[1, 0] >= 0
    own, _ = bank.search([bank.row(4)], 1, native=native)
    assert own.tolist() == [[4]]                                    # a row is its own nearest neighbour
    for bad in (lambda: bank.search(entries, 0, native=native), lambda: bank.search(entries, 17, native=native),
                lambda: bank.search(torch.zeros(2, SIZE + 1), 1, native=native), lambda: bank.search(torch.zeros(2, SIZE, dtype=torch.float64), 1, native=native),
                lambda: bank.search(entries, 2, exclude=['first'], native=native), lambda: bank.search([], 1, native=native)):
        with pytest.raises(ValueError):
            bad()


def test_song_means_and_neighbours():
    """song_means: one row per song in by_song's order, the float32 loop of bank.song(s)'s weights, provenance (song, 0, summed
    bars); neighbours: the means searched with the song's own mean, itself excluded."""
    native = simutil.sim_native()
    bank, rows = filled_bank()
    means = bank.song_means(native=native)
    songs = ['first', 7, 'second', 'third']
    assert len(means) == 4 and list(means.by_song) == songs and means.style_size == SIZE
    assert means.provenance == [('first', 0, 2 + 3 + 3), (7, 0, 2 + 2), ('second', 0, 3 + 3), ('third', 0, 2)]
    want = []
    for s in songs:
        entries = bank.song(s)
        acc = entries[0][1] * rows[entries[0][0]]
        for r, w in entries[1:]:
            acc = acc + w * rows[r]
        assert acc.dtype == np.float32
        want.append(acc)
    want = np.stack(want)
    assert np.array_equal(sb.words(means.rows[:4]).reshape(4, SIZE), want.view(np.uint32))
    assert np.array_equal(sb.words(means.rows[3]), rows[6].view(np.uint32))                  # one window: the mean is the row
    c32 = sc.chain(want, want)
    for farthest in (False, True):
        for g, s in enumerate(songs):
            got = bank.neighbours(s, 2, farthest=farthest, native=native)
            ranked = sc.ranking(c32[g], np.arange(4) != g, 2, -1 if farthest else 1)
            assert [name for name, _ in got] == [songs[r] for r in ranked] and s not in [name for name, _ in got]
            assert [np.float32(x) for _, x in got] == c32[g, ranked].tolist()
    assert len(bank.neighbours('third', 16, native=native)) == 3                             # fewer other songs than k
    with pytest.raises(KeyError):
        bank.neighbours('nowhere', 1, native=native)
    from style.data import StyleBank
    assert len(StyleBank(SIZE, 'cpu').song_means(native=native)) == 0


def test_nearest_validation_and_too_few_foreign_rows():
    from style.data import Nearest
    n = Nearest()
    assert (n.k, n.exclude_own, n.farthest, n.order) == (1, True, False, 1) and Nearest(16, False, True).order == -1
    assert repr(Nearest(3, farthest=True)) == 'Nearest(k=3, exclude_own=True, farthest=True)'
    for bad in (0, -1, 17, 2.5, '3', None, True):
        with pytest.raises(ValueError):
            Nearest(bad)
    bank, _ = filled_bank()                                          # 8 rows: 3 of 'first', 2 of 7, 2 of 'second', 1 of 'third'
    assert bank.exclusions(Nearest(5), ['first', 7, 'nowhere']) == [0, 1, -1]
    assert bank.exclusions(Nearest(8, exclude_own=False), ['first', 7]) == [-1, -1]
    assert bank.exclusions(Nearest(6), [7, 'third', 'nowhere']) == [1, 3, -1]
    assert bank.exclusions(Nearest(8), ['nowhere']) == [-1]
    for nearest, songs in ((Nearest(6), ['third', 'first']), (Nearest(7), [7]), (Nearest(9, exclude_own=False), ['first']), (Nearest(9), ['nowhere'])):
        with pytest.raises(ValueError, match='fewer than'):
            bank.exclusions(nearest, songs)
