#!/usr/bin/env python3
"""Pair alignment maps (store.alignment_map_for_pairs: per word the best region, per region the best word, csrc/rescore.hip)
against the re-score call they share a main loop with, at COCO-1k store sizes (1000 x 5000): the stores of tools/bench_rerank.py
(synth.eval_sets-style lengths, D = 768, split), k = 50, both directions.  Prints ONE JSON line.

Per direction, on one matching-head shortlist: alignment_map_for_pairs with all outputs, the same call with words=True,
regions=False, and the comparator alignment_scores_for_pairs (the existing re-score call, never the new one).  The number of
interest is by how much the same main loop plus the arg-max epilogues and their writes exceeds the re-score time.

Protocol (tools/bench_rerank.py's): one process; a clock-settling pre-roll; then `--rounds` rounds (>= 5) in which the paths
alternate, each timed over `--calls` calls between two HIP events; per path the median of the rounds' per-call times, min / max as
the spread.  There is no fallback: without an MI355X this fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PATHS = ('alignment_map_for_pairs', 'alignment_map_for_pairs words only', 'alignment_scores_for_pairs')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--preroll-s', type=float, default=1.0)
    ap.add_argument('--n-img', type=int, default=1000, help='images in the store; captions are 5 x')
    ap.add_argument('--D', type=int, default=768)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--precision', default='split')
    args = ap.parse_args()
    import torch
    from aladin_amd import evaluation as E
    from aladin_amd.store import alignment_map_for_pairs, alignment_scores_for_pairs
    from bench_rerank import build_stores
    if not torch.cuda.is_available():
        raise SystemExit('bench_align_map: needs the MI355X (no GPU visible, no fallback)')
    dev = torch.device('cuda:0')

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def summary(ms):
        return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
                'spread_ms': round(max(ms) - min(ms), 4)}

    si, sc = build_stores(args.n_img, args.D, args.precision, dev)
    out = {'tool': 'bench_align_map', 'shape': [len(si), len(sc), args.D], 'k': args.k, 'precision': args.precision, 'rounds': args.rounds,
           'calls_per_round': args.calls, 'preroll_s': args.preroll_s, 'device': torch.cuda.get_device_name(0),
           'max_regions': si.max_count(), 'max_words': sc.max_count(), 'directions': {}}
    for direction in ('i2t', 't2i'):
        short, _ = E.search_topk(si, sc, args.k, direction)
        fns = (lambda: alignment_map_for_pairs(si, sc, short, direction),
               lambda: alignment_map_for_pairs(si, sc, short, direction, words=True, regions=False),
               lambda: alignment_scores_for_pairs(si, sc, short, direction))
        full = fns[0]()
        assert torch.equal(full.score.view(torch.int32), fns[2]().view(torch.int32)), 'the map\'s score is not the re-score call\'s'
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.preroll_s:
            for fn in fns:
                fn()
            torch.cuda.synchronize()
        t = {name: [] for name in PATHS}
        for _ in range(args.rounds):
            for name, fn in zip(PATHS, fns):
                t[name].append(timed(fn, args.calls))
        r = {name: summary(ms) for name, ms in t.items()}
        base = r[PATHS[2]]
        for name in PATHS[:2]:
            r[name]['over_rescore_ms'] = round(r[name]['median_ms'] - base['median_ms'], 4)
            r[name]['over_rescore_ratio'] = round(r[name]['median_ms'] / base['median_ms'], 3)
            r[name]['difference_over_larger_spread'] = round((r[name]['median_ms'] - base['median_ms'])
                                                             / max(r[name]['spread_ms'], base['spread_ms'], 1e-6), 2)
        r['pairs'] = int((short >= 0).sum())
        r['output_bytes'] = sum(v.numel() * v.element_size() for v in full)
        out['directions'][direction] = r
    print(json.dumps(out))


if __name__ == '__main__':
    main()
