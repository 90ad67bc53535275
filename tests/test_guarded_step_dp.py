"""The guarded optimizer step under data parallelism, world size 2 on CPU (gloo): per-rank gradients are all-reduced with SUM
first, so the guard sees the summed gradient and every rank takes the same decision — clip coefficient and skip alike — and
lands on the bits one process gets from the summed gradient.  Kernels: the product's .hip sources on the hipsim interpreter."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4099 + 1025          # two slices of the norm kernel and a ragged one


def _grads(rank, round_):
    import guard_cases as gc
    g = gc.mixed(N, 100 + 10 * round_ + rank) * np.float32(1e-13)
    if round_ == 1 and rank == 1:
        g[N // 2] = np.nan                      # a bad song on rank 1 only
    return g


def _run(lib, summed):
    """Three guarded steps (clipped, skipped, clipped) over the already summed gradients; returns the buffers."""
    import guard_cases as gc
    b = gc.Bufs(lib, N, seed=9)
    for g in summed:
        b.set_grads(g)
        assert b.guarded(.25, 1) == 0
    return b


def _worker(rank, world, port, out):
    for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'music-style-transfer_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import guard_cases as gc
    from simutil import sim_native
    lib = sim_native().lib
    b = gc.Bufs(lib, N, seed=9)                 # the same parameters on every rank
    skipped = []
    for round_ in range(3):
        b.set_grads(_grads(rank, round_))
        dist.all_reduce(b.g, op=dist.ReduceOp.SUM)              # sum, not mean — what FusedAdam.step does before the guard
        assert b.guarded(.25, 1) == 0
        skipped.append(float(b.guard[2]))
    mine = torch.cat([b.p, b.m, b.v, b.state, b.guard])
    gathered = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(gathered, mine)
    if rank == 0:
        torch.save(dict(ranks=gathered, skipped=skipped), out)
    dist.destroy_process_group()


def test_two_ranks_take_the_same_guarded_decision(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import guard_cases as gc
    from simutil import sim_native
    lib = sim_native().lib                       # build the interpreter library once, before forking
    out = str(tmp_path / 'guard_dp.pt')
    port = 30500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    r = torch.load(out)
    assert gc.same_bits(r['ranks'][0], r['ranks'][1]), 'ranks diverged after the guarded steps'
    assert r['skipped'] == [0., 1., 0.]          # the NaN on rank 1 alone made BOTH ranks skip
    one = _run(lib, [gc.effective(_grads(0, k), _grads(1, k)) for k in range(3)])       # one process, the summed gradient
    want = torch.cat([one.p, one.m, one.v, one.state, one.guard])
    assert gc.same_bits(r['ranks'][0], want)
    guard = one.guard.numpy()
    assert guard[3] == 1 and guard[4] == 2 and float(one.state[0]) == 2
