#!/usr/bin/env python3
"""A/B of two CHECKOUTS on the no-grad alignment grid, on ONE box in one session (tools/ab_bench.py explains why): for a change
of the host code that drives the grid (aladin_amd/eval_grid.py), where both checkouts run the same library.  The checkouts
alternate (and swap their order from one alternation to the next), every measurement is `tools/bench_eval.py --alignment-only`
of that checkout in a fresh process, `--reps` alternations (default 5).  Rule per row, as in tools/ab_retrieval.py: the branch's
median over the alternations <= the yardstick's median + the yardstick's own max - min.

    python tools/ab_eval_grid.py OUT.json parent=/path/to/parent/checkout branch=. [--reps N]

A checkout without a built library takes ALADIN_LIB from the environment.  Stops at the first child that fails or runs out of
time: nothing more is started on the GPU after that."""
import json
import os
import statistics
import subprocess
import sys


def rows_of(lines):
    """{row name: ms} of one run's JSON lines."""
    return {d['workload']: d['ms'] for d in lines}


def main():
    args = sys.argv[1:]
    reps = int(args.pop(args.index('--reps') + 1)) if '--reps' in args else 5
    args = [a for a in args if a != '--reps']
    out_path, trees = args[0], [a.split('=', 1) for a in args[1:]]
    raw = {name: {} for name, _ in trees}
    for rep in range(reps):
        for name, path in (trees if rep % 2 == 0 else trees[::-1]):       # A B, B A, ...: neither checkout always runs on the warmer chip
            r = subprocess.run([sys.executable, os.path.join(os.path.abspath(path), 'tools', 'bench_eval.py'), '--alignment-only'],
                               capture_output=True, text=True, timeout=400)
            if r.returncode != 0:
                raise SystemExit('bench_eval.py of %s failed (%d): %s' % (name, r.returncode, r.stderr[-600:]))
            got = rows_of([json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')])
            for k, v in got.items():
                raw[name].setdefault(k, []).append(v)
            print(rep, name, got, flush=True)
    yard = trees[0][0]
    rows, ok = {}, True
    for name, _ in trees[1:]:
        for k, y in raw[yard].items():
            v = raw[name][k]
            rows['%s: %s' % (name, k)] = {'yardstick_median': statistics.median(y), 'yardstick_spread': max(y) - min(y), 'median': statistics.median(v),
                                          'pass': statistics.median(v) <= statistics.median(y) + (max(y) - min(y))}
            ok &= rows['%s: %s' % (name, k)]['pass']
    res = {'rule': 'median <= yardstick median + (yardstick max - yardstick min), %d alternations in one session' % reps, 'yardstick': yard,
           'raw': raw, 'rows': rows, 'all_pass': ok}
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    for k, r in rows.items():
        print('%s\n    %s  %.3f vs %.3f + %.3f' % (k, 'pass' if r['pass'] else 'FAIL', r['median'], r['yardstick_median'], r['yardstick_spread']))
    print('all pass:', ok)


if __name__ == '__main__':
    main()
