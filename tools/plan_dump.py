#!/usr/bin/env python3
"""What the scheduler decided, one JSON line per plan: tiling, workspace, zero lists and, for every stage mask and both passes,
each step's shape, carrier reports, launch count and GEMM members ({M, N, K, k-splits, folded rows, workgroups, kernel
variant, k-tile depth} each, in the order the launch dispatches them).  Plans are built by the CPU interpreter library (no GPU);
run it before and after a change to the scheduler and diff the two outputs."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'music-style-transfer_amd'), os.path.join(ROOT, 'tests')]
from parity_cases import FULL, SMALL      # noqa: E402
from simutil import make_dims, sim_native      # noqa: E402
from style._native import PlanOptions      # noqa: E402

K_GEMM, K_GEMM_FOLD = 0, 25
# (name, widths, (C, R, T), clips, plan options): the shapes of the rider tests, then every kind of plan that carries nothing
CASES = [('full_4_16_4', FULL, (4, 16, 4), 1, {}), ('full_2_7_2', FULL, (2, 7, 2), 1, {}), ('small_3_2_3', SMALL, (3, 2, 3), 1, {}),
         ('small_4_3_3', SMALL, (4, 3, 3), 1, {}), ('small_2_2_2_x3', SMALL, (2, 2, 2), 3, {}),
         ('full_2_4_2_no_merge', FULL, (2, 4, 2), 1, dict(no_merge=1)), ('full_2_4_2_branches', FULL, (2, 4, 2), 1, dict(branches=1)),
         ('full_2_4_2_tile64', FULL, (2, 4, 2), 1, dict(gemm_tile=64)), ('full_2_4_2_tiled', FULL, (2, 4, 2), 1, dict(tile_r0=0, tile_rows=2)),
         ('small_2_2_2_x8', SMALL, (2, 2, 2), 8, {}), ('full_7_8_10_x64', FULL, (7, 8, 10), 64, {})]


def dump(lib, name, widths, crt, clips, opts):
    dims, st = make_dims(widths, *crt, unpitched=True, clips=clips), C.c_int32()
    plan = lib.mst_plan_create_ex(C.byref(dims), C.byref(PlanOptions(**opts)), C.byref(st))
    assert plan, (name, st.value)
    row = dict(case=name, gemm_tile=lib.mst_plan_gemm_tile(plan), workspace_floats=lib.mst_plan_workspace_floats(plan),
               zero_rides=lib.mst_plan_zero_rides(plan), zero_floats={m: lib.mst_plan_zero_floats(plan, m) for m in (7, 1, 2, 4)})
    for mask in (7, 1, 2, 4):
        for bwd in (0, 1):
            n = lib.mst_plan_step_count(plan, mask, bwd)
            info, gemms, kinds = np.zeros((n, 8), np.int32), np.zeros((4096, 6), np.int32), np.zeros((4096, 2), np.int32)
            assert lib.mst_plan_step_info(plan, mask, bwd, info.ctypes.data) == n
            cols = {}
            for what in ('carried', 'riders', 'carrier'):
                out = np.full(n, -9, np.int32)
                assert getattr(lib, 'mst_plan_step_' + what)(plan, mask, bwd, out.ctypes.data) == n
                cols['step_' + what] = out.tolist()
            members = []
            for i in range(n):
                m = lib.mst_plan_step_gemms(plan, mask, bwd, i, gemms.ctypes.data, len(gemms))
                assert lib.mst_plan_step_gemm_kinds(plan, mask, bwd, i, kinds.ctypes.data, len(kinds)) == m
                members.append(np.concatenate([gemms[:m], kinds[:m]], axis=1).tolist())
            assert all(bool(m) == (k in (K_GEMM, K_GEMM_FOLD)) for m, k in zip(members, info[:, 5].tolist()))
            row['mask%d_%s' % (mask, 'bwd' if bwd else 'fwd')] = dict(step_info=info.tolist(), launch_count=lib.mst_plan_launch_count(plan, mask, bwd),
                                                                   step_gemms=members, **cols)
    lib.mst_plan_destroy(plan)
    return json.dumps(row, sort_keys=True)


if __name__ == '__main__':
    lib = sim_native().lib
    for case in CASES:
        print(dump(lib, *case))
