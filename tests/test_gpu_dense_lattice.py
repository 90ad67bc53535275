"""-m gpu: every entry of the width lattice (lattice_cases.LATTICE) on the hipcc/gfx950 build on a real MI355X against the oracle
evaluated in FLOAT64: lin.hip at every (kernel family x width residue) cell, at 32 and 35 rows per clip and across the lin16
routing, conv.hip at OC = 64, 33, 32 and the accessor GEMM at OC = 65, and the default routing on the same ragged widths.
tests/test_dense_lattice.py asserts what the lattice contains; here each entry is one small plan and the one-thread oracle."""
import pytest
import torch

import lattice_cases as lc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def native():
    from style import _native as nat
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return nat.get()       # raises if libmst_amd.so is missing: no fallback


@pytest.mark.parametrize('i', range(len(lc.LATTICE)))
def test_lattice_entry_against_float64(native, i):
    lc.run(native, DEV, lc.LATTICE[i], tag=lc.tag(i))
