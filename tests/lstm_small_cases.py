"""Shared by test_lstm_small.py (CPU interpreter) and test_gpu_lstm_small.py: the one-wave LSTM kernels of hidden sizes up to 16
(csrc/lstm.hip, lstm_fwd_small_kernel / lstm_bwd_small_kernel) against the register-flavour kernels they replace, bit for bit.
The default plan takes the one-wave kernels; the same plan scheduled with no_merge = 1 and set_lstm_small(0) launches every LSTM
member on its own lstm_fwd_kernel<true> / lstm_bwd_kernel<true>, the path of the parent commit."""
import combine_rider_cases as cr

K_GEMM, K_LSTM_F, K_LSTM_B = 0, 3, 4
SMALL_H = 16         # LSTM_SH: largest hidden size of the one-wave flavour
RIDE_H = 8           # LSTM_RIDE_H: largest hidden size of a backward recurrence a gemm_kernel launch carries
MST_ERR_UNSUPPORTED = -2


def lstm_rows(plan, backward, mask=7):
    """[(index, row)] of the LSTM recurrence steps of a pass; row = {B, S, H, multi, count, kind, level, chain}"""
    return [(i, r) for i, r in enumerate(cr.step_rows(plan, backward, mask)) if r[5] in (K_LSTM_F, K_LSTM_B)]


def small_steps(plan, backward):
    return [(i, r) for i, r in lstm_rows(plan, backward) if r[2] <= SMALL_H]


def pair(native, device, widths, C, R, T, clips=1):
    a = cr.Run(native, device, widths, C, R, T, clips)
    b = cr.Run(native, device, widths, C, R, T, clips, no_merge=1)
    b.plan.set_lstm_small(0)
    assert all(c == -1 for backward in (False, True) for c in b.plan.step_carrier(7, backward))
    for backward in (False, True):
        assert small_steps(a.plan, backward), 'the case has no LSTM launch of a hidden size the one-wave kernels take'
    return a, b


def small_equals_register_flavour(native, device, widths, C, R, T, clips=1):
    a, b = pair(native, device, widths, C, R, T, clips)
    for it in range(2):          # the first on a poisoned workspace, the second on what the first left
        a.iterate(poison=it == 0)
        b.iterate(poison=it == 0)
        cr.assert_same(a, b)
    return a, b


def expect_reports(plan, mixes=True):
    """A backward LSTM step of hidden sizes <= 8 whose level has a GEMM launch is run by that launch (plans that mix kinds in a
    launch); every other LSTM step has a launch of its own; the two older reports stay 0 for LSTM steps; every carried step names
    a GEMM step of its own level, and the launch count is lower by the carried LSTM steps.  Returns how many LSTM steps ride."""
    riding = 0
    for backward in (False, True):
        rows = cr.step_rows(plan, backward)
        carrier, carried, riders = plan.step_carrier(7, backward), plan.step_carried(7, backward), plan.step_riders(7, backward)
        assert len(carrier) == len(rows)
        for i, r in enumerate(rows):
            if r[5] in (K_LSTM_F, K_LSTM_B):
                assert (carried[i], riders[i]) == (0, 0), r
                gemm_levels = {g[6] for g in rows if g[5] == K_GEMM}
                if mixes and r[5] == K_LSTM_B and r[2] <= RIDE_H and r[6] in gemm_levels:
                    g = rows[carrier[i]]
                    assert carrier[i] >= 0 and g[5] == K_GEMM and g[6] == r[6], (r, carrier[i])
                    riding += 1
                else:
                    assert carrier[i] == -1, r
            elif riders[i]:
                g = rows[carrier[i]]
                assert carrier[i] >= 0 and g[5] == K_GEMM and g[6] == r[6] and carrier[carrier[i]] == -1, (r, carrier[i])
            else:
                assert carrier[i] == -1, r
        # every step without a carrier is at least one launch; a backward pass ends with one slab reduction per stage
        own = sum(c == -1 for c in carrier) + (3 if backward else 0)
        assert plan.launch_count(7, backward) >= own
    return riding
