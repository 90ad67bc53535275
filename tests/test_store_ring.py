"""The rotating song store on the CPU: mst_store_admit (the product's kernel source on the hipsim interpreter, the cases of
tests/admit_cases.py), `style.data.ring_place`, and the ring mode of style.data.SongStore on the host — a scripted and a seeded
random admit sequence with the ring's invariants after every step, what evicted ids do, and the two together: the script
through the kernel, cropped by mst_clip_window."""
import numpy as np
import pytest
import torch

import admit_cases as ac
import simutil


@pytest.mark.parametrize('case', ac.CASES, ids=[c.__name__[5:] for c in ac.CASES])
def test_store_admit(case):
    case(simutil.sim_native(), 'cpu')


def test_ring_place_against_a_brute_force_model():
    from style.data import ring_place
    capacity = 64
    for head in range(capacity + 1):
        for count in range(capacity + 1):
            fits = [f for f in range(head, head + 4) if f % 4 == 0 and f + count <= capacity]
            first = fits[0] if fits else 0
            assert ring_place(head, count, capacity) == (first, first + count), (head, count)
            assert first % 4 == 0 and first + count <= capacity


def test_scripted_admit_sequence_on_the_host():
    """A wrap in each pool, an admit that evicts several songs, a song that ends exactly at `capacity`, a group of three, and the
    refusals (too large, alone and inside a group; no pitched notes) that leave pools, tables and bookkeeping as they were."""
    store = ac.run_script('cpu')
    assert len(store.resident()) <= ac.RESIDENT < len(store)


def test_seeded_random_admit_sequence():
    from style.data import SongStore
    rng = np.random.default_rng(12)
    palette = [ac.clip(k, *spec) for k, spec in enumerate([ac.MEDIUM, ac.SMALL, ac.MEDIUM, ac.MEDIUM, ac.SMALL, ac.BIG])]
    palette += [ac.clip(8, 2, 2, 1, percussion=False), ac.clip(40, 1, 3, 2), ac.clip(41, 2, 2, 2, percussion=False), ac.clip(42, 1, 5, 1)]
    capacity = max(c.pitched_channels.count for c in palette) + 150      # the largest song fits, hardly two of them
    resident = 5
    store = SongStore('cpu', capacity=capacity, resident=resident)
    sources, admits = {}, 0
    while admits < 200:
        group = [palette[int(i)] for i in rng.integers(0, len(palette), int(rng.integers(1, 4)))]
        ids = store.admit(group) if len(group) > 1 or rng.integers(2) else [store.add(group[0])]
        assert ids == list(range(len(sources), len(sources) + len(group)))
        sources.update(zip(ids, group))
        admits += len(group)
        ac.verify(store, sources, capacity, resident)
    assert len(store) == admits and len(set(store.resident())) == len(store.resident())
    assert all(b['table'].shape[0] == 16 for b in store.buckets.values())       # rows were reused: no table ever grew
    store.check()


def _after_evictions():
    from style.data import SongStore
    clips = [ac.clip(k, *ac.MEDIUM) for k in (0, 2, 3, 9, 10, 11)] + [ac.clip(8, 2, 2, 1, percussion=False)]
    store = SongStore('cpu', capacity=sum(c.pitched_channels.count for c in clips[:3]) + 16, resident=4)
    store.admit(clips[:3])
    return store, clips


def test_evicted_songs_are_never_named_and_refused_when_named():
    from style.data import SongEvicted, WindowBatch
    store, clips = _after_evictions()
    stale = store.sample(np.random.default_rng(0), 4, 2)
    assert set(stale.songs.tolist()) <= {0, 1, 2}
    all_windows = store.window_batches(2, 3)
    store.admit(clips[3:])
    live = store.resident()
    assert len(store) == 7 and live and set(live) < set(range(7)) and store.evicted(0) and not store.evicted(6)
    assert issubclass(SongEvicted, LookupError)
    rng = np.random.default_rng(1)
    for _ in range(30):
        assert set(store.sample(rng, 3, 2).songs.tolist()) <= set(live)
    assert {s for s, _ in store.windows(2, 1)} == set(live)
    assert {int(s) for batch, _ in store.window_batches(2, 3) for s in batch.songs} == set(live)
    # a batch drawn before the refresh fails loudly, before anything is written
    gone = [s for s in stale.songs.tolist() if store.evicted(s)]
    assert gone
    out = np.full((2, 4, 4), 7, np.int32)
    with pytest.raises(SongEvicted):
        store.describe(stale, out)
    with pytest.raises(SongEvicted):
        store.small_inputs(stale)
    for batch, _ in all_windows:
        if any(store.evicted(int(s)) for s in batch.songs):
            with pytest.raises(SongEvicted):
                store.describe(batch, out)
    for call in (lambda: store.bucket_of(gone[0]), lambda: store.window_sounds(gone[0], 0, 2)):
        with pytest.raises(SongEvicted):
            call()
    assert store.songs[gone[0]] is None
    with pytest.raises(IndexError):
        store.describe(WindowBatch(2, 2, 1, True, [len(store)], [0]), out)


def test_an_append_only_store_is_what_it_was():
    """resident=None: `add` places songs back to back, unaligned, the pools grow by doubling, no song is ever evicted, and the
    ring's entry points say so."""
    from style.data import SongStore
    clips = [ac.clip(k, *ac.MEDIUM) for k in (0, 2, 3)] + [ac.clip(1, *ac.SMALL)]
    store = SongStore('cpu', capacity=64)
    at = {5: 0, 2: 0}
    for k, c in enumerate(clips):
        assert store.add(c) == k
        for name, nfeat, roll in (('pitched', 5, c.pitched_channels), ('unpitched', 2, c.unpitched_channels)):
            assert store.songs[k][name] == (at[nfeat], roll.count)
            at[nfeat] += roll.count
    assert any(store.songs[k]['pitched'][0] % 4 for k in range(4))
    assert store.pools[5].cells.numel() > 64 and store.pools[5].used == at[5]
    assert store.resident() == [0, 1, 2, 3] and not any(store.evicted(k) for k in range(4))
    assert all(b['table'].shape[1] == b['fields'][-1][1] for b in store.buckets.values())
    store.check()
    with pytest.raises(ValueError):
        store.admit(clips[:1])


def test_refresh_schedule():
    """style.train.Rotation: the first N usable songs make the ring, every E-th iteration admits the next M; a song without
    pitched notes (None) is skipped, one too large for the ring is skipped and counted, and a source that runs out ends the
    refreshing."""
    from style.train import Rotation, train
    big = ac.clip(6, 2, 5, 2, density=.12)
    order = [ac.clip(0, *ac.MEDIUM), None, ac.clip(1, *ac.SMALL), ac.clip(2, *ac.MEDIUM), big, ac.clip(3, *ac.MEDIUM), None, ac.clip(4, *ac.SMALL),
             ac.clip(9, *ac.MEDIUM), big, ac.clip(10, *ac.MEDIUM)]
    rotation = Rotation(iter(order), every=3, count=2)
    store = rotation.first_store(3, records=big.pitched_channels.count - 1)
    assert store.resident() == [0, 1, 2] and store.capacity == big.pitched_channels.count - 1 and rotation.too_large == 0
    seen = {}
    for iteration in range(12):
        rotation.after(iteration)
        seen[iteration] = store.resident()
    assert seen[0] == seen[1] == [0, 1, 2] and seen[2] == seen[4] == [2, 3, 4] and seen[5] == seen[7] == [4, 5, 6]
    assert seen[8] == seen[11] == [4, 5, 6] and rotation.exhausted and rotation.too_large == 2 and len(store) == 7
    store.check()
    # the default ring: twice the larger pool's records of the first songs, rounded up to a power of two
    clips = [c for c in order if c is not None and c is not big]
    store = Rotation(iter(clips), 1, 1).first_store(3)
    total = sum(c.pitched_channels.count for c in clips[:3])
    assert store.capacity >= 2 * total > store.capacity // 2 and store.capacity & (store.capacity - 1) == 0
    for bad in (dict(refresh_every=2), dict(refresh_every=0, batch_clips=3), dict(refresh_every=2, batch_clips=3, refresh_songs=0),
                dict(refresh_every=2, batch_clips=3, store_records=0)):
        with pytest.raises(ValueError):
            train(None, iter(()), n_iterations=1, training_info_path=None, save_path=None, progress=False, **bad)


def test_script_through_the_kernel():
    ac.case_ring_crops_equal_the_append_only_store(simutil.sim_native(), 'cpu')
