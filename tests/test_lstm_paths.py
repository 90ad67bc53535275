"""The LSTM recurrences' memory paths (csrc/lstm.hip) on the CPU interpreter: the multi-workgroup backward's LDS-staged operands
and joint poll of a lane's three granules against the single-workgroup flavour, the joint poll's failure contract, and the
register flavour's 16-byte weight load and early first-chunk fetch against the oracle.  (FULL widths on the interpreter:
10-70 s per case.)"""
import pytest
import torch

import parity_cases as pc
from tools.synth import synth_clip
from simutil import sim_native
from style import _native as nat
from test_lstm_multi import lstm_steps, run


@pytest.mark.parametrize('R', [2, 5])      # one exchanged step (the smallest case of the joint poll); both buffer parities twice
def test_multi_equals_single_workgroup_flavour(R):
    native = sim_native()
    C, T = 1, 1
    dims = pc.make_dims(pc.FULL, C, R, T, True)
    flat, _, _ = pc.random_params(native, dims)
    clip = synth_clip(3, C, R, T, True, density=0.05)
    multi = nat.Plan(native, dims, 'cpu')
    single = nat.Plan(native, dims, 'cpu', lstm_flavour=1)
    assert [s[3] for s in lstm_steps(multi)] == [1] and [s[3] for s in lstm_steps(multi, True)] == [1]
    assert [s[3] for s in lstm_steps(single)] == [0] and [s[3] for s in lstm_steps(single, True)] == [0]
    g1, l1 = run(multi, flat, clip)
    g0, l0 = run(single, flat, clip)
    assert multi.status() == 0 and single.status() == 0
    assert torch.isfinite(l1[0, 0]) and torch.equal(l1.nan_to_num(-1.), l0.nan_to_num(-1.))
    assert torch.equal(multi.view('style'), single.view('style'))
    assert torch.equal(g1, g0)


def test_joint_poll_keeps_the_failure_contract():
    native = sim_native()
    C, R, T = 1, 2, 1
    dims = pc.make_dims(pc.FULL, C, R, T, True)
    flat, _, _ = pc.random_params(native, dims)
    clip = synth_clip(3, C, R, T, True, density=0.05)
    plan = nat.Plan(native, dims, 'cpu', lstm_flavour=2)          # workgroup 0 publishes its first step under a wrong epoch
    assert [s[3] for s in lstm_steps(plan)] == [2]
    g, losses = run(plan, flat, clip)
    assert torch.isnan(losses[0, 0])
    assert plan.status(clear=False) == nat.DEV_LSTM_TIMEOUT
    assert plan.status() == nat.DEV_LSTM_TIMEOUT and plan.status() == 0
    ok = nat.Plan(native, dims, 'cpu')
    g, losses = run(ok, flat, clip)
    assert ok.status() == 0 and torch.isfinite(losses[0, 0]) and torch.isfinite(g).all()


@pytest.mark.parametrize('w,C,R,T', [
    (pc.FULL, 1, 2, 2),       # register flavour at H = 64, 9 and 8, S = 2
    (pc.SMALL, 2, 3, 2),      # small hidden sizes that are no multiple of 4: rows that are not 16-byte aligned
])
def test_register_flavour_matches_the_oracle(w, C, R, T):
    e, worst = pc.oracle_case(sim_native(), 'cpu', w, C, R, T, True, check_bitwise=True)
    print('all-gradient rel-L2', e, 'worst tensor', worst)
