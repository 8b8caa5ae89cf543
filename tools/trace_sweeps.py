#!/usr/bin/env python3
"""Per-sweep digest of a rocprofv3 --kernel-trace capture of one streaming equalisation loop (tuning aid).

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/pmc_unit.py --batch 64 --sweeps 24 --le-only
    python tools/trace_sweeps.py DIR/.../t_kernel_trace.csv --store 8

Prints the launches of the LAST loop of the capture (from its le_prepare_kernel on), sweep by sweep, and the mean duration of
le_level_kernel by the kind of sweep: lazy (the deferred layers are not read), reading (the last sweep of a 4-sweep window that
does not store), storing (the last sweep of a store period of --store sweeps).  The start of a launch is stamped where the
previous one ends, so a launch boundary is part of the duration of the launch behind it."""
import argparse
import csv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('csv')
    ap.add_argument('--store', type=int, default=8, help='store period of the deferred layers (LEPlan.store_depth)')
    ap.add_argument('--window', type=int, default=4, help='read / verdict window (LEPlan.defer_depth)')
    ap.add_argument('--group', type=int, default=8, help='group depth of the free-running layers')
    ap.add_argument('--skip', type=int, default=2, help='sweeps left out of the means (cold code and tables)')
    a = ap.parse_args()
    rows = list(csv.DictReader(open(a.csv)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    first = max(i for i, r in enumerate(rows) if 'le_prepare_kernel' in r['Kernel_Name'])
    short = lambda r: r['Kernel_Name'].split('(')[0].split('<')[0].split('::')[-1]
    dur = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    sweeps, cur, head, tail = [], {}, [], []
    for r in rows[first:]:
        n = short(r)
        if n in ('le_lean_kernel', 'le_level_kernel', 'le_control_kernel'):
            if tail:
                break                               # (a later loop)
            cur[n] = cur.get(n, 0.0) + dur(r)
            cur.setdefault('t0', int(r['Start_Timestamp']))
            if n == 'le_control_kernel':
                cur['total'] = (int(r['End_Timestamp']) - cur['t0']) / 1e3
                sweeps.append(cur)
                cur = {}
        elif not sweeps and not cur:
            head.append((n, dur(r)))
        else:
            tail.append((n, dur(r)))
    print('launches in front of the first sweep: ' + ', '.join('{} {:.1f}'.format(n, d) for n, d in head))
    print('per sweep (us); F = first of a group (le_lean_kernel in front), R = reads the deferred layers, S = stores them, '
          'G = last of a group')
    kinds = {}
    for k, s in enumerate(sweeps):
        reads = k % a.window == a.window - 1
        stores = k % a.store == a.store - 1
        flags = ('F' if k % a.group == 0 else '-') + ('S' if stores else 'R' if reads else '-') + ('G' if k % a.group == a.group - 1 else '-')
        print('  sweep {:2d} {} total {:7.1f}  lean {:6.1f}  level {:6.1f}  control {:5.1f}'.format(
            k, flags, s['total'], s.get('le_lean_kernel', 0.0), s['le_level_kernel'], s['le_control_kernel']))
        if k >= a.skip:
            kind = 'storing' if stores else 'reading' if reads else 'lazy'
            for key in (kind, 'all'):
                kinds.setdefault(key, []).append(s)
    print('launches behind the last sweep: ' + ', '.join('{} {:.1f}'.format(n, d) for n, d in tail))
    print('means over sweeps {}..{} (us)'.format(a.skip, len(sweeps) - 1))
    for kind in ('lazy', 'reading', 'storing', 'all'):
        ss = kinds.get(kind, [])
        if ss:
            m = lambda key: sum(s.get(key, 0.0) for s in ss) / len(ss)
            print('  {:8s} n={:2d}  level {:6.1f}  control {:5.1f}  lean (per sweep) {:5.1f}  sweep {:6.1f}'.format(
                kind, len(ss), m('le_level_kernel'), m('le_control_kernel'), m('le_lean_kernel'), m('total')))


if __name__ == '__main__':
    main()
