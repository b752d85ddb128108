#!/usr/bin/env python3
"""Gallery index search (ops.search_index_topk on a prebuilt ops.build_search_index) against ops.search_topk on the same tensors:
gallery 25000 x 768 in both directions with n_q in {1, 8, 32, 256, 5000}, gallery 589824 x 768 with n_q in {1, 8, 32, 256}
(dim = 1), k = 50.  Prints ONE JSON line.

Protocol (tools/bench_search.py's): one process; a clock-settling pre-roll; then `--rounds` rounds (>= 5) in which the two paths
alternate, each timed over a number of calls between two HIP events; per path the median of the rounds' per-call times, with
min / max as the spread.  A one-pass row (n_q <= 32) passes when the index path's median is below search_topk's by more than the
larger spread; a tile-route row passes when its median is at most search_topk's plus that spread.  Build time and bytes stand
apart: the index, the index search's workspace, aladin_search_workspace_bytes.  For the large gallery the one-pass rows also give
the gallery bytes per second of the whole call and an ESTIMATE for the streaming pass alone -- not a kernel timing: the call's
time minus that of the same call on a 16-item index (packing, selection and the final gather at the same n_q), beside the 6.0-6.3 TB/s copy rate of the MI355X.
There is no fallback: without an MI355X this fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_TBS = (6.0, 6.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--budget-ms', type=float, default=150.0, help='calls per timing = what fits this many ms (at least 3, at most 50)')
    ap.add_argument('--preroll-s', type=float, default=0.5)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--D', type=int, default=768)
    ap.add_argument('--small-gallery', type=int, default=25000)
    ap.add_argument('--large-gallery', type=int, default=589824)
    ap.add_argument('--skip-large', action='store_true')
    args = ap.parse_args()
    import torch
    from aladin_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit('bench_index: needs the MI355X (no GPU visible, no fallback)')
    if args.rounds < 5:
        raise SystemExit('bench_index: at least 5 rounds')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    D, k = args.D, args.k

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def preroll(fns):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.preroll_s:
            for fn in fns:
                fn()
            torch.cuda.synchronize()

    def calls_for(fn):
        fn()
        torch.cuda.synchronize()
        return max(3, min(50, int(args.budget_ms / max(timed(fn, 2), 1e-3))))

    def summary(ms):
        return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
                'spread_ms': round(max(ms) - min(ms), 4)}

    def alternate(fa, fb):
        preroll([fa, fb])
        ca, cb = calls_for(fa), calls_for(fb)
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(fa, ca))
            tb.append(timed(fb, cb))
        return summary(ta), summary(tb)

    def randn(n, seed):
        g = torch.Generator().manual_seed(seed)
        return torch.randn((n, D), generator=g).to(dev)

    out = {'tool': 'bench_index', 'D': D, 'k': k, 'rounds': args.rounds, 'preroll_s': args.preroll_s,
           'device': torch.cuda.get_device_name(0), 'stream_max_q': ops.SEARCH_INDEX_STREAM_MAX_Q, 'copy_rate_tbs': list(COPY_RATE_TBS),
           'galleries': []}
    tiny = ops.build_search_index(randn(16, 5))
    plans = [(args.small_gallery, (1, 0), (1, 8, 32, 256, 5000))]
    if not args.skip_large:
        plans.append((args.large_gallery, (1,), (1, 8, 32, 256)))
    for n_g, dims, n_qs in plans:
        gallery = randn(n_g, 1)
        index = ops.build_search_index(gallery)
        torch.cuda.synchronize()
        build = summary([timed(lambda: ops.build_search_index(gallery), 2) for _ in range(args.rounds)])
        gal_bytes = n_g * 4 * D                                         # the packed rows one pass reads: [hi | lo] fp16
        entry = {'gallery': [n_g, D], 'index_bytes': int(lib.aladin_search_index_bytes(n_g, D)), 'build': build, 'rows': []}
        for dim in dims:
            for n_q in n_qs:
                q = randn(n_q, 100 + n_q)
                img, cap = (q, gallery) if dim == 1 else (gallery, q)
                f_index = lambda: ops.search_index_topk(index, q, k, dim=dim)                  # noqa: E731
                f_topk = lambda: ops.search_topk(img, cap, k, dim=dim)                         # noqa: E731
                assert torch.equal(f_index(), f_topk()), 'the two paths disagree'
                s_i, s_t = alternate(f_index, f_topk)
                spread = max(s_i['spread_ms'], s_t['spread_ms'])
                one_pass = n_q <= ops.SEARCH_INDEX_STREAM_MAX_Q and D <= ops.SEARCH_INDEX_STREAM_MAX_D
                row = {'dim': dim, 'n_q': n_q, 'route': 'one-pass' if one_pass else 'tile', 'index': s_i, 'search_topk': s_t,
                       'speedup': round(s_t['median_ms'] / s_i['median_ms'], 3),
                       'passes': bool(s_i['median_ms'] < s_t['median_ms'] - spread) if one_pass
                       else bool(s_i['median_ms'] <= s_t['median_ms'] + spread),
                       'index_workspace_bytes': int(lib.aladin_search_index_workspace_bytes(n_q, n_g, D, k, dim)),
                       'search_topk_workspace_bytes': int(lib.aladin_search_workspace_bytes(*((n_q, n_g) if dim == 1 else (n_g, n_q)), D, k, dim))}
                if one_pass and n_g == args.large_gallery:
                    f_tiny = lambda: ops.search_index_topk(tiny, q, k, dim=dim)                # noqa: E731
                    preroll([f_tiny])
                    c = calls_for(f_tiny)
                    rest = statistics.median([timed(f_tiny, c) for _ in range(args.rounds)])
                    kernel_ms = max(s_i['median_ms'] - rest, 1e-6)
                    row['call_tbs'] = round(gal_bytes / (s_i['median_ms'] * 1e-3) / 1e12, 3)
                    row['rest_of_call_ms'] = round(rest, 4)
                    row['stream_pass_estimate_tbs'] = round(gal_bytes / (kernel_ms * 1e-3) / 1e12, 3)
                    row['stream_pass_estimate_fraction_of_copy_rate'] = round(row['stream_pass_estimate_tbs'] / COPY_RATE_TBS[0], 3)
                entry['rows'].append(row)
                del q, img, cap
        out['galleries'].append(entry)
        del gallery, index
        torch.cuda.empty_cache()
    out['all_pass'] = all(r['passes'] for g in out['galleries'] for r in g['rows'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
