#!/usr/bin/env python3
"""Top-k gallery search (ops.search_topk) against the stored path (ops.sim_matrix + ops.topk_indices) at evaluation scale:
5000 x 25000 x 768 on synth.retrieval_embeddings(sigma=8), k = 50, both directions, and the 70 x 40000 x 64 gallery the
stored top-k refuses (time only).  Prints ONE JSON line.

Protocol: one process; a clock-settling pre-roll; then `--rounds` rounds (>= 5) in which the two paths alternate, each timed
over `--calls` calls (>= 20) between two HIP events; per path the median of the rounds' per-call times, with min / max as the
spread.  Peak workspace bytes stand beside the times: what each path allocates besides the inputs and the (n_q, k) outputs.
There is no fallback: without an MI355X this fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--preroll-s', type=float, default=1.0)
    ap.add_argument('--n-img', type=int, default=5000)
    ap.add_argument('--D', type=int, default=768)
    ap.add_argument('--k', type=int, default=50)
    args = ap.parse_args()
    import torch
    from aladin_amd import _lib, ops, synth
    if not torch.cuda.is_available():
        raise SystemExit('bench_search: needs the MI355X (no GPU visible, no fallback)')
    dev = torch.device('cuda:0')
    lib = _lib.load()
    img_rows, cap_rows = synth.retrieval_embeddings(args.n_img, args.D, sigma=8.0)
    img = torch.from_numpy(img_rows[0::5].copy()).to(dev)
    cap = torch.from_numpy(cap_rows).to(dev)
    n_img, n_cap, D, k = img.shape[0], cap.shape[0], args.D, args.k

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

    def summary(ms):
        return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
                'spread_ms': round(max(ms) - min(ms), 4)}

    out = {'tool': 'bench_search', 'shape': [n_img, n_cap, D], 'k': k, 'sigma': 8.0, 'rounds': args.rounds, 'calls_per_round': args.calls,
           'preroll_s': args.preroll_s, 'device': torch.cuda.get_device_name(0), 'dims': {}}
    for dim in (1, 0):
        fused = lambda: ops.search_topk(img, cap, k, dim=dim)                               # noqa: E731
        stored = lambda: ops.topk_indices(ops.sim_matrix(img, cap), k, dim=dim)             # noqa: E731
        assert torch.equal(fused(), stored()), 'the two paths disagree'
        preroll([fused, stored])
        t_f, t_s = [], []
        for _ in range(args.rounds):
            t_f.append(timed(fused, args.calls))
            t_s.append(timed(stored, args.calls))
        f, s = summary(t_f), summary(t_s)
        f['workspace_bytes'] = int(lib.aladin_search_workspace_bytes(n_img, n_cap, D, k, dim))
        s['workspace_bytes'] = int(lib.aladin_sim_workspace_bytes(n_img, n_cap, D)) + n_img * n_cap * 4       # + the score matrix
        out['dims'][str(dim)] = {'search_topk': f, 'sim_matrix+topk_indices': s,
                                 'speedup': round(s['median_ms'] / f['median_ms'], 3),
                                 'difference_over_larger_spread': round((s['median_ms'] - f['median_ms']) / max(f['spread_ms'], s['spread_ms'], 1e-6), 2)}
    # the gallery the stored top-k refuses: 70 queries x 40000 items x 64
    g = torch.Generator().manual_seed(31)
    q, gal = torch.randn((70, 64), generator=g).to(dev), torch.randn((40000, 64), generator=g).to(dev)
    big = {}
    for dim, (a, b) in ((1, (q, gal)), (0, (gal, q))):
        fn = lambda: ops.search_topk(a, b, k, dim=dim)                                      # noqa: E731
        preroll([fn])
        big[str(dim)] = summary([timed(fn, args.calls) for _ in range(args.rounds)])
        big[str(dim)]['workspace_bytes'] = int(lib.aladin_search_workspace_bytes(a.shape[0], b.shape[0], 64, k, dim))
    out['gallery_40000'] = {'shape': [70, 40000, 64], 'dims': big}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
