#!/usr/bin/env python3
"""A/B of two library builds on the evaluation similarity paths, on ONE box in one session (tools/ab_bench.py explains why): the
builds alternate (and swap their order from one alternation to the next), every measurement in a fresh process with ALADIN_LIB set, `--reps` alternations.  Rows: every timing
tools/bench_search.py (--rounds 5 --calls 20), tools/bench_retrieval.py (--only synth) and tools/bench_eval.py (--matching-only)
report.  Rule per row: the branch's median over the alternations <= the yardstick's median + the yardstick's own max - min.

    python tools/ab_retrieval.py OUT.json parent=OLD.so branch=aladin_amd/lib/libaladin_hip.so

Stops at the first child that fails or runs out of time: nothing more is started on the GPU after that."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = (('bench_search.py', '--rounds', '5', '--calls', '20'), ('bench_retrieval.py', '--only', 'synth'), ('bench_eval.py', '--matching-only'))


def rows_of(tool, lines):
    """{row name: ms} of one run's JSON lines."""
    out = {}
    for d in lines:
        if tool == 'bench_search.py':
            for dim, paths in d['dims'].items():
                for path in ('search_topk', 'sim_matrix+topk_indices'):
                    out['search 5000x25000 dim%s %s ms' % (dim, path)] = paths[path]['median_ms']
            for dim, s in d['gallery_40000']['dims'].items():
                out['search 70x40000 dim%s search_topk ms' % dim] = s['median_ms']
        elif tool == 'bench_retrieval.py':
            name = d['data'].split(' = ')[0]
            out['retrieval %s fused ms' % name], out['retrieval %s all-exact ms' % name] = d['fused_ms'], d['fused_all_exact_ms']
        else:
            for key in ('sim_ms', 'rank_ms', 'fused_sim_plus_rank_ms'):
                out['eval matching head %s' % key] = d[key]
    return out


def main():
    reps = 5
    out_path, libs = sys.argv[1], [a.split('=', 1) for a in sys.argv[2:]]
    raw = {name: {} for name, _ in libs}
    for rep in range(reps):
        for tool in TOOLS:
            for name, path in (libs if rep % 2 == 0 else libs[::-1]):       # A B, B A, ...: neither build always runs on the warmer chip
                env = dict(os.environ, ALADIN_LIB=os.path.abspath(path))
                r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', tool[0])] + list(tool[1:]), env=env, capture_output=True, text=True,
                                   timeout=240)
                if r.returncode != 0:
                    raise SystemExit('%s with %s failed (%d): %s' % (tool[0], name, r.returncode, r.stderr[-600:]))
                got = rows_of(tool[0], [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')])
                for k, v in got.items():
                    raw[name].setdefault(k, []).append(v)
                print(rep, name, tool[0], got, flush=True)
    yard = libs[0][0]
    rows, ok = {}, True
    for name, _ in libs[1:]:
        for k, y in raw[yard].items():
            v = raw[name][k]
            bound = statistics.median(y) + (max(y) - min(y))
            rows['%s: %s' % (name, k)] = {'yardstick_median': statistics.median(y), 'yardstick_spread': max(y) - min(y), 'median': statistics.median(v),
                                          'pass': statistics.median(v) <= bound}
            ok &= rows['%s: %s' % (name, k)]['pass']
    res = {'rule': 'median <= yardstick median + (yardstick max - yardstick min), %d alternations in one session' % reps, 'yardstick': yard,
           'raw': raw, 'rows': rows, 'all_pass': ok}
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    for k, r in rows.items():
        print('%-90s %s  %.4f vs %.4f + %.4f' % (k, 'pass' if r['pass'] else 'FAIL', r['median'], r['yardstick_median'], r['yardstick_spread']))
    print('all pass:', ok)


if __name__ == '__main__':
    main()
