#!/usr/bin/env python3
"""Every LSTM launch of a rocprofv3 --kernel-trace run per kernel and grid: tools/lstm_launch_stats.py <dir> [name]
(`name`: another substring of the kernel name, e.g. gemm_kernel, instead of lstm).  Prints calls and the average / median / min / max / 10th / 90th percentile duration in us (a merged launch shows as one
grid: Grid_Size_Y counts its members)."""
import collections, csv, glob, sys
f = glob.glob(sys.argv[1] + '/*/*kernel_trace.csv')[0]
pat = sys.argv[2] if len(sys.argv) > 2 else 'lstm'
d = collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    n = r['Kernel_Name'].split('(')[0].replace('void ', '')
    if pat in n:
        d[(n, r.get('Grid_Size_X', '?'), r.get('Grid_Size_Y', '?'))].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
for k, v in sorted(d.items()):
    v.sort()
    avg = sum(v) / len(v)
    print(f'{k[0]:28s} grid {k[1]:>6s} x {k[2]:>3s} calls {len(v):5d} avg {avg:7.2f} med {v[len(v) // 2]:7.2f} min {v[0]:7.2f} max {v[-1]:7.2f} p10 {v[len(v) // 10]:7.2f} p90 {v[len(v) * 9 // 10]:7.2f}')
