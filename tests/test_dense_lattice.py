"""The width lattice of lattice_cases on the hipsim CPU interpreter: what LATTICE has to contain is asserted here for EVERY entry
through plan creation alone (milliseconds per plan), and a subset runs numerically against the float64 oracle.

Entries that run numerically here: SIM_RUN = 0 and 5.  Together they hold the K = 1 and K = 3 (mod 4) weight-gradient cells of
all three weight-gradient kernels, the forward 2 x 2 kernel at K = 3 (mod 4) and conv.hip at its limit OC = 64 and its
minimum P = 8 (entry 0) - the cells the mutation checks of DESIGN.md 4.1 need - at the smallest widths and shapes of the
lattice.  The other entries do not run here: interpreter time grows with the widths (2 - 3 minutes for an entry at
(2, 4, 4) x 2 clips with bar widths of 200 - 270, against 30 - 50 s for these two), and tests/test_gpu_dense_lattice.py runs
every entry on the card, which is where the code generation differs."""
import pytest

import lattice_cases as lc
import parity_cases as pc
from simutil import make_dims, sim_native
from style import _native as nat

SIM_RUN = [0, 5]


@pytest.fixture(scope='module')
def plans():
    native = sim_native()
    return [lc.make_plan(native, 'cpu', e) for e in lc.LATTICE]


def test_lattice_reaches_every_cell_of_the_linear_kernels(plans):
    native = sim_native()
    # the lin.hip plans of the other test files (parity_cases.FULL / SMALL, all on gemm_tile = 64, dense_flavour = 2)
    old = set()
    for w, C, R, T, clips in [(pc.FULL, 3, 4, 2, 5), (pc.FULL, 7, 3, 3, 1), (pc.FULL, 2, 3, 2, 1), (pc.SMALL, 3, 3, 1, 3)]:
        old |= lc.lin_cells(nat.Plan(native, make_dims(w, C, R, T, True, clips=clips), 'cpu', **lc.FORCED))
    new = set().union(*[lc.lin_cells(plans[i]) for i in lc.FORCED_ENTRIES])
    print(f'lin.hip cells: {len(old)} of {len(lc.ALL_CELLS)} in the FULL / SMALL plans, {len(new)} in the lattice')
    assert old <= lc.ALL_CELLS and new <= lc.ALL_CELLS
    assert not [c for c in old if c[-1] in (1, 3)], 'the FULL / SMALL plans were taken to have no odd K'
    unreachable = {c for c, reason in lc.UNREACHABLE}
    assert len(unreachable) <= 4 and not [c for c in unreachable if c[-1] in (1, 3)]
    assert not unreachable & new, 'a cell listed as unreachable is reached'
    assert new == lc.ALL_CELLS - unreachable, sorted(lc.ALL_CELLS - unreachable - new)
    assert len(new) > len(old)


def test_lattice_stays_inside_its_limits(plans):
    assert len({tuple(sorted(e[0].items())) for e in lc.LATTICE}) <= 10
    for (w, C, R, T, clips, opts), plan in zip(lc.LATTICE, plans):
        assert w['melody'] in (4, 8, 12, 16)
        assert (C <= 7 and R <= 3 and T <= 3) or (C <= 2 and R <= 4 and T <= 4) or (C, R, T) == (5, 7, 1), (C, R, T)
        assert C * R * T <= 63 and 1 <= clips <= 6
        hidden = [r[2] for r in lc.step_rows(plan, False) if r[5] == 3]          # K_LSTM_F: {B, S, H, multi}
        assert hidden and max(hidden) <= 256, hidden


def test_row_edges(plans):
    forced = [(lc.LATTICE[i], lc.lin_steps(plans[i])) for i in lc.FORCED_ENTRIES]
    # rows = 32 exactly: the routing gate of plan.hip's linear()
    assert [1 for e, steps in forced if any(s[1] == 32 for s in steps)]
    # 35 rows per clip, 3 clips: 32-row k-tiles and row tiles straddle the clip boundaries
    assert [1 for e, steps in forced if e[4] == 3 and {lc.K_LIN_F, lc.K_LIN_A, lc.K_LIN_W} <= {s[0] for s in steps if s[1] == 35}]
    # pitched_rhythm_encoder.channels_linear (K = 280) on both sides of the lin16 routing
    for N in (16, 17):
        assert [1 for e, steps in forced if {(lc.K_LIN_F, N, 280), (lc.K_LIN_W, N, 280)} <= {(s[0], s[2], s[3]) for s in steps}], N


def conv_out_channels(entry):
    w, C, R, T, clips, opts = entry
    table = sim_native().param_table(make_dims(w, C, R, T, True))
    return next(shape[0] for name, off, shape in table if name == 'pitched_channels_encoder.beats_conv.module.weight')


def test_conv_edges(plans):
    assert [conv_out_channels(e) for e in lc.LATTICE[:4]] == [64, 33, 32, 65]
    assert lc.LATTICE[3][0]['beat'] == 79
    for i in range(4):
        assert lc.LATTICE[i][4] > 1 and i in lc.FORCED_ENTRIES
        kinds = lc.step_kinds(plans[i])
        assert ({lc.K_CONV_P, lc.K_CONV_F, lc.K_CONV_W} <= kinds) == (i < 3), (i, sorted(kinds))
        assert (lc.K_CONV_F in kinds) == (i < 3)
    assert [1 for w, C, R, T, clips, opts in lc.LATTICE[:3] if C * R * T in (8, 9)]


def test_default_routing_entries(plans):
    lin_conv = {lc.K_CONV_F, lc.K_LIN_F, lc.K_LIN_A, lc.K_LIN_W}
    defaults = [i for i, e in enumerate(lc.LATTICE) if not {k for k in e[5] if k != 'seed'}]
    assert len(defaults) == 2
    forced_widths = [lc.LATTICE[i][0] for i in lc.FORCED_ENTRIES]
    one, six = sorted(defaults, key=lambda i: lc.LATTICE[i][4])
    for i in defaults:
        assert lc.LATTICE[i][0] in forced_widths
    assert lc.LATTICE[one][4] == 1 and plans[one].gemm_tile == 32 and not lin_conv & lc.step_kinds(plans[one])
    assert lc.LATTICE[six][4] == 6 and plans[six].gemm_tile == 64 and lc.K_CONV_F in lc.step_kinds(plans[six])


def test_interpreter_subset_holds_the_odd_weight_gradient_cells(plans):
    cells = set().union(*[lc.lin_cells(plans[i]) for i in SIM_RUN])
    for family in lc.DW_FAMILIES:
        for k in (1, 3):
            assert [c for c in cells if c[0] == 'dw' and c[1] == family and c[3] == k], (family, k)
    assert ('fwd', 'rows<2,2,0>', 3) in cells
    assert [i for i in SIM_RUN if lc.K_CONV_F in lc.step_kinds(plans[i]) and conv_out_channels(lc.LATTICE[i]) == 64]


@pytest.mark.parametrize('i', SIM_RUN)
def test_lattice_entry_against_float64(i):
    lc.run(sim_native(), 'cpu', lc.LATTICE[i], tag=lc.tag(i))
