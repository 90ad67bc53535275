"""-m gpu: the guarded optimizer step on an MI355X — the C ABI cases of tests/test_guarded_step.py at a small size and at the
full-width model's flat size, one captured graph replayed over an ordinary, a clipped and a skipped step, and the Python
surface (FusedAdam(max_grad_norm=..., skip_nonfinite=...), guard_stats, grad_norms) on the two accumulation lanes."""
import numpy as np
import pytest
import torch

import guard_cases as gc
from tools.synth import synth_clip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = (1025, 980325)          # one ragged slice; the seed-108 full-width model's parameter count


@pytest.fixture(scope='module')
def lib():
    from style import _native
    return _native.get().lib


@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('two', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_norm(lib, n, two, lead):
    b = gc.Bufs(lib, n, DEV, two=two, lead=lead)
    g, g2 = gc.mixed(n, 1), (gc.mixed(n, 2) if two else None)
    b.set_grads(g, g2)
    got, again = b.norm(), b.norm()
    want = gc.arbiter_norm(g, g2)
    print(n, two, lead, got, want, gc.ulps(got, want))
    assert gc.ulps(got, want) <= 1
    assert got.view(np.int32) == again.view(np.int32)


@pytest.mark.parametrize('two', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_clip_is_scale_then_the_existing_step_bitwise(lib, n, two):
    gc.check_clip_is_scale_then_step(lib, n, DEV, two)


@pytest.mark.parametrize('zero_grad', [0, 1])
@pytest.mark.parametrize('n', SIZES)
def test_nonfinite_step_is_skipped(lib, n, zero_grad):
    for name, g, g2 in gc.nonfinite_cases(n):
        gc.check_skip(lib, n, DEV, name, g, g2, zero_grad)


def test_one_captured_graph_replays_ordinary_clipped_and_skipped_steps(lib):
    n = SIZES[1]
    b = gc.Bufs(lib, n, DEV, two=True, seed=4)
    ref = b.clone()
    g, g2 = gc.mixed(n, 50) * np.float32(1e-10), gc.mixed(n, 51) * np.float32(1e-10)
    max_norm = 2 * float(gc.arbiter_norm(g, g2))
    warm = b.clone()
    assert warm.guarded(max_norm, 1) == 0            # loads the code objects: capturing executes nothing
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                    # one chain on the capture stream, no forked streams
        assert b.guarded(max_norm, 1) == 0
    bad = g.copy()
    bad[12345] = np.nan
    rounds = [('ordinary', g, g2), ('clipped', g * np.float32(1e6), g2 * np.float32(1e6)), ('skipped', bad, g2)]
    for name, x, x2 in rounds:
        b.set_grads(x, x2)
        graph.replay()
        guard = b.guard.cpu().numpy()
        if name == 'ordinary':
            assert guard[1] == 1 and guard[2] == 0
        elif name == 'clipped':
            assert 0 < guard[1] < 1 and guard[2] == 0
        else:
            assert guard[1] == 0 and guard[2] == 1
        if name != 'skipped':                        # the arbiter: an unguarded step on host-scaled gradients
            ref.set_grads(gc.effective(x, x2) * np.float32(guard[1]))
            assert ref.plain() == 0
        assert b.same_optimizer(ref), name
        assert not b.g.any() and not b.g2.any()
    guard = b.guard.cpu().numpy()
    assert guard[3] == 1 and guard[4] == 1 and float(b.state[0]) == 2
    assert gc.ulps(guard[5], gc.arbiter_norm(g * np.float32(1e6), g2 * np.float32(1e6))) <= 1


def test_fused_adam_guard_on_the_two_lanes():
    from style.optim import FusedAdam
    from test_gpu_model_surface import load_small, to_dev
    z, model = load_small('small_unpitched')
    _, twin = load_small('small_unpitched')
    C, R, T = (int(v) for v in z['crt'])
    clips = [to_dev(synth_clip(k, C, R, T, True, density=float(z['density']))) for k in (0, 1, 2)]
    args = lambda c: (c['mode'], c['bpm'], c['pitched'], c['instruments_features'], c['unpitched'], c['used_instruments'], c['bpm_int'])
    opt, opt_twin = FusedAdam(model, max_grad_norm=1.), FusedAdam(twin)
    iterate = lambda m: [m.train_iteration(*args(c)) for c in clips[:2]]      # two accumulation iterations, one per lane
    iterate(model)
    norms = opt.grad_norms()                         # waits for the lanes without consuming them
    assert list(norms) == list(model.state_dict())
    total = np.sqrt(np.sum(np.asarray(list(norms.values()), dtype=np.float64) ** 2))
    assert np.isfinite(total) and total > 0
    opt.max_grad_norm = float(total) / 2             # M: half the norm, so this step is clipped
    opt.step()
    stats = opt.guard_stats()
    print(stats, total)
    assert gc.ulps(np.float32(total), stats['norm']) <= 4        # both <= 1 ulp from exact; the rest is the fp32 recombination here
    assert 0 < stats['coef'] < 1 and stats['steps_clipped'] == 1 and not stats['skipped']
    # the twin runs after the model is done: models of one shape share the cached plan's workspaces, lane by lane
    torch.cuda.synchronize()
    iterate(twin)
    g2 = twin.join_lanes()
    assert g2 is not None
    twin._gflat.add_(g2)
    g2.zero_()
    twin._gflat.mul_(stats['coef'])
    opt_twin.step()
    assert gc.same_bits(model._flat, twin._flat) and gc.same_bits(opt.exp_avg_sq, opt_twin.exp_avg_sq)
    assert not model._gflat.any()
    # a clip whose bpm input is NaN: the step is skipped, the parameters stay
    opt.skip_nonfinite = True
    before = model._flat.clone()
    poisoned = dict(clips[2], bpm=torch.full_like(clips[2]['bpm'], float('nan')))
    model.train_iteration(*args(poisoned))
    opt.step()
    stats = opt.guard_stats()
    assert stats['skipped'] and stats['steps_skipped'] == 1 and not np.isfinite(stats['norm'])
    assert gc.same_bits(model._flat, before) and float(opt.state[0]) == 1
    assert not model._gflat.any()
    model.train_iteration(*args(clips[2]))           # the next good step proceeds
    opt.step()
    stats = opt.guard_stats()
    assert not stats['skipped'] and stats['steps_skipped'] == 1 and np.isfinite(stats['norm']) and float(opt.state[0]) == 2
    assert not gc.same_bits(model._flat, before) and bool(torch.isfinite(model._flat).all())
