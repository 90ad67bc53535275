"""The one-wave LSTM kernels (H <= 16: one wave per sequence, no workgroup barrier, one LDS exchange per step) on
the CPU interpreter build: bit for bit against the register-flavour kernels over two train iterations, against the oracle, and
what the plan reports about them."""
import pytest

import lstm_small_cases as ls
import parity_cases as pc
from simutil import sim_native
from style import _native as nat


# FULL 2,5,2: H = 9 with B = 5, S = 2 and H = 8 with S = 5; FULL 1,2,1: S = 1 and S = 2, the first-step paths (c_prev = 0, no
# recurrent gradient yet); SMALL 3,2,3: H = 8, 3 and other sizes that are no multiple of 4, the reverse direction of the
# bidirectional bars LSTM, several members per launch; SMALL 2,7,2 x 2 clips: the launches of a two-clip plan; SMALL 2,3,2 x 6
# clips: a batched plan on the 64x64 tiling whose small LSTM launches hold too few sequences for the grouped flavour
@pytest.mark.parametrize('widths,C,R,T,clips', [(pc.FULL, 2, 5, 2, 1), (pc.FULL, 1, 2, 1, 1), (pc.SMALL, 3, 2, 3, 1),
                                                (pc.SMALL, 2, 7, 2, 2), (pc.SMALL, 2, 3, 2, 6)])
def test_one_wave_kernels_equal_the_register_flavour_bit_for_bit(widths, C, R, T, clips):
    ls.small_equals_register_flavour(sim_native(), 'cpu', widths, C, R, T, clips)


def test_small_widths_cover_hidden_sizes_off_the_chain_length():
    plan = nat.Plan(sim_native(), pc.make_dims(pc.SMALL, 3, 2, 3, True), 'cpu')
    sizes = {r[2] for backward in (False, True) for _, r in ls.small_steps(plan, backward)}
    assert any(h % 4 for h in sizes) and 8 in sizes, sizes


@pytest.mark.parametrize('widths,C,R,T', [(pc.FULL, 2, 5, 2), (pc.SMALL, 2, 3, 2)])
def test_oracle(widths, C, R, T):
    pc.oracle_case(sim_native(), 'cpu', widths, C, R, T, True, check_bitwise=True)


def test_lstm_steps_keep_their_own_launches_and_reports():
    native = sim_native()
    plan = nat.Plan(native, pc.make_dims(pc.FULL, 4, 16, 4, True), 'cpu')
    assert ls.expect_reports(plan) == 1               # the bars LSTM's backward (H = 8, level 5) rides; its forward shares its level with no GEMM launch
    assert plan.launch_count(7, False) == 30 and plan.launch_count(7, True) == 38          # 30 / 39 with every LSTM step on its own launch
    for backward in (False, True):
        small = ls.small_steps(plan, backward)
        assert sorted(r[2] for _, r in small) == [8, 9], small            # the bars and the beats LSTM of the song-info model
        assert any(c >= 0 for c in plan.step_carrier(7, backward))         # gathers / segment reduces / combines name their GEMM step
    assert plan.lib.mst_plan_set_lstm_small(plan.handle, 0) == ls.MST_ERR_UNSUPPORTED      # a GEMM launch runs an LSTM step
    unmerged = nat.Plan(native, pc.make_dims(pc.FULL, 4, 16, 4, True), 'cpu', no_merge=1)
    assert ls.expect_reports(unmerged, mixes=False) == 0
    assert unmerged.launch_count(7, True) > plan.launch_count(7, True)
    assert unmerged.lib.mst_plan_set_lstm_small(unmerged.handle, 0) == 0 and unmerged.lib.mst_plan_set_lstm_small(unmerged.handle, 1) == 0


def test_small_widths_carry_two_backward_recurrences():
    plan = nat.Plan(sim_native(), pc.make_dims(pc.SMALL, 3, 2, 3, True), 'cpu')
    assert ls.expect_reports(plan) == 2               # H = 3 and H = 2 beside a GEMM launch; the H = 8 one has none on its level


@pytest.mark.parametrize('clips,opts', [(1, dict(gemm_tile=64)), (1, dict(branches=1)), (1, dict(no_merge=1)),
                                        (1, dict(tile_r0=0, tile_rows=2)), (8, dict())])
def test_other_plans_report_no_carrier(clips, opts):
    plan = nat.Plan(sim_native(), pc.make_dims(pc.FULL, 4, 16, 4, True, clips=clips), 'cpu', **opts)
    if clips > 1:
        assert plan.gemm_tile == 64
    for mask in (7, 1, 2, 4):
        for backward in (False, True):
            assert all(c == -1 for c in plan.step_carrier(mask, backward))
    assert plan.lib.mst_plan_set_lstm_small(plan.handle, 0) == 0


def test_step_carrier_per_stage_lists_index_their_own_list():
    plan = nat.Plan(sim_native(), pc.make_dims(pc.FULL, 2, 4, 2, True), 'cpu')
    for mask in (1, 2, 4):
        for backward in (False, True):
            rows, carrier, riders = ls.cr.step_rows(plan, backward, mask), plan.step_carrier(mask, backward), plan.step_riders(mask, backward)
            assert len(rows) == len(carrier)
            for r, c, k in zip(rows, carrier, riders):
                assert (c >= 0) == (k != 0) or r[5] == ls.K_LSTM_B, (r, c, k)
                if c >= 0:
                    assert rows[c][5] == ls.K_GEMM and rows[c][6] == r[6]
