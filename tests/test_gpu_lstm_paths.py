"""-m gpu: the LSTM recurrences' memory paths (csrc/lstm.hip) on an MI355X: staged operands across chunk boundaries, the early
first-chunk fetch with the unchanged refills, the 16-byte weight load, and the multi-workgroup exchange with its joint poll
against the single-workgroup flavour."""
import pytest
import torch

import parity_cases as pc
from tools.synth import synth_clip
from style import _native as nat
from test_lstm_multi import lstm_steps

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FULL = pc.FULL


@pytest.fixture(scope='module')
def native():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return nat.get()       # raises if libmst_amd.so is missing: no fallback


@pytest.mark.parametrize('C,R,T', [
    (1, 40, 1),      # S = 40 bars: over the H = 64 forward chunk (32 steps) once, the backward one (18) twice; 39 exchanged steps
    (2, 2, 1),       # S = 2: one exchange, B > 1 on the beat LSTMs
])
def test_lstm_paths_match_the_oracle(native, C, R, T):
    e, worst = pc.oracle_case(native, DEV, FULL, C, R, T, True, check_bitwise=True)
    print((C, R, T), 'all-gradient rel-L2', e, 'worst tensor', worst)


def test_multi_equals_single_workgroup_flavour(native):
    C, R, T = 1, 5, 1
    dims = pc.make_dims(FULL, C, R, T, True)
    flat, _, _ = pc.random_params(native, dims)
    clip = synth_clip(3, C, R, T, True, density=0.05)
    out = []
    for flavour in (0, 1):
        plan = nat.Plan(native, dims, DEV, lstm_flavour=flavour)
        assert [s[3] for s in lstm_steps(plan)] == [1 - flavour] and [s[3] for s in lstm_steps(plan, True)] == [1 - flavour]
        pc.set_clip(plan, clip)
        g = torch.zeros_like(flat, device=DEV)
        losses = torch.zeros(nat.N_LOSSES, device=DEV)
        xp, xu = pc.dev_clip(clip, DEV)
        pc.poison(plan)
        plan.train_iteration(flat.to(DEV), g, xp, xu, losses)
        torch.cuda.synchronize()
        assert plan.status() == 0
        out.append((losses.cpu(), plan.view('style').cpu().clone(), g.cpu()))
    (l1, s1, g1), (l0, s0, g0) = out
    assert torch.isfinite(l1[0]) and torch.equal(l1.nan_to_num(-1.), l0.nan_to_num(-1.))
    assert torch.equal(s1, s0)
    assert torch.equal(g1, g0)
