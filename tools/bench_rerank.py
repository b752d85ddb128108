#!/usr/bin/env python3
"""Two-stage retrieval (evaluation.search_rerank: matching-head shortlist + alignment-head re-scoring of its pairs) at COCO-1k
(1000 x 5000) and COCO-5k (5000 x 25000) store sizes: synth.eval_sets-style lengths (11-33 regions, 4-27 scored words), D = 768,
split stores, k = 50, both directions.  Prints ONE JSON line.

Per size and direction: search_rerank end to end, the re-score kernel alone (ops.align_rescore on a fixed shortlist, with its rate
at 2 * R' * T' * D * 3 flop per pair -- R', T' the pair's region / word counts rounded up to the 16-row MFMA tiles -- against the
2.5 PF fp16 peak) and, at COCO-1k only, the comparator: the alignment grid compute_sim_matrix(stores, mode='alignment') +
ops.topk_indices, the only way to the same answer without the re-score kernel.  Beside the times: how often the re-ranked top-1 /
top-10 differ from the matching-head shortlist's (synthetic data: says nothing about COCO).

Protocol: one process; a clock-settling pre-roll; then `--rounds` rounds (>= 5) in which the paths alternate, each timed over
`--calls` calls between two HIP events; per path the median of the rounds' per-call times, min / max as the spread.
There is no fallback: without an MI355X this fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP16_FLOPS = 2.5e15


def build_stores(n_img, D, precision, dev, seed=31, batch=500):
    """n_img images and 5 * n_img captions in two PackedSetStores: lengths as synth.eval_sets draws them, sets = a per-image base
    direction + unit noise (generated on the device batch by batch: the (N, 71, 768) host arrays of eval_sets would be 5 GB)."""
    import torch
    from aladin_amd import synth
    from aladin_amd.store import PackedSetStore
    N = 5 * n_img
    img_len = [int(v) for v in synth.integers((n_img,), 12, 34, seed + 1)]
    cap_len = [int(v) for v in synth.integers((N,), 7, 30, seed + 2)]
    g_img, g_cap = synth.retrieval_embeddings(n_img, D, seed + 6, sigma=3.0)
    gen = torch.Generator(device=dev).manual_seed(seed)
    base = 0.25 * torch.randn((n_img, 1, D), generator=gen, device=dev)
    si = PackedSetStore(D, 0, dev, capacity_rows=sum(img_len), precision=precision)
    sc = PackedSetStore(D, 2, dev, capacity_rows=sum(cap_len), precision=precision)
    for k0 in range(0, n_img, batch):
        k1 = min(n_img, k0 + batch)
        sets = torch.randn((k1 - k0, max(img_len[k0:k1]), D), generator=gen, device=dev) + base[k0:k1]
        si.append(sets, img_len[k0:k1], torch.from_numpy(g_img[5 * k0:5 * k1:5].copy()).to(dev))
    for k0 in range(0, N, batch):
        k1 = min(N, k0 + batch)
        owner = torch.arange(k0, k1, device=dev) // 5
        sets = torch.randn((k1 - k0, max(cap_len[k0:k1]), D), generator=gen, device=dev) + base[owner]
        sc.append(sets, cap_len[k0:k1], torch.from_numpy(g_cap[k0:k1].copy()).to(dev))
    return si, sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--grid-calls', type=int, default=5)
    ap.add_argument('--preroll-s', type=float, default=1.0)
    ap.add_argument('--sizes', default='1000,5000', help='images per store; captions are 5 x')
    ap.add_argument('--grid-up-to', type=int, default=1000, help='largest size at which the alignment grid is timed')
    ap.add_argument('--D', type=int, default=768)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--precision', default='split')
    args = ap.parse_args()
    import torch
    from aladin_amd import evaluation as E
    from aladin_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('bench_rerank: needs the MI355X (no GPU visible, no fallback)')
    dev = torch.device('cuda:0')
    k, D = args.k, args.D

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

    out = {'tool': 'bench_rerank', 'D': D, 'k': k, 'precision': args.precision, 'rounds': args.rounds, 'calls_per_round': args.calls,
           'grid_calls_per_round': args.grid_calls, 'preroll_s': args.preroll_s, 'device': torch.cuda.get_device_name(0), 'sizes': {}}
    for n_img in [int(v) for v in args.sizes.split(',')]:
        si, sc = build_stores(n_img, D, args.precision, dev)
        oi, ci = si._tables()
        oc, cc = sc._tables()
        x = (si.rows, oi, ci, None, len(si), si.max_count())
        y = (sc.rows, oc, cc, None, len(sc), sc.max_count())
        res = {'shape': [len(si), len(sc), D], 'store_bytes': si.nbytes() + sc.nbytes(), 'directions': {}}
        for direction in ('i2t', 't2i'):
            dim = 1 if direction == 'i2t' else 0
            short, _ = E.search_topk(si, sc, k, direction)
            buf = torch.empty(short.shape, dtype=torch.float32, device=dev)
            two_stage = lambda: E.search_rerank(si, sc, k, direction)                                        # noqa: E731
            kernel = lambda: ops.align_rescore(x, y, short, dim, D, args.precision, si.padded_len - 1, out=buf)      # noqa: E731
            with_grid = n_img <= args.grid_up_to
            grid = lambda: ops.topk_indices(E.compute_sim_matrix(si, sc, mode='alignment'), k, dim=dim)      # noqa: E731
            idx, val = two_stage()
            fns = [two_stage, kernel] + ([grid] if with_grid else [])
            preroll(fns)
            t = {name: [] for name in ('search_rerank', 'rescore_kernel', 'alignment_grid+topk_indices')}
            for _ in range(args.rounds):
                t['search_rerank'].append(timed(two_stage, args.calls))
                t['rescore_kernel'].append(timed(kernel, args.calls))
                if with_grid:
                    t['alignment_grid+topk_indices'].append(timed(grid, args.grid_calls))
            r = {name: summary(ms) for name, ms in t.items() if ms}
            # the kernel's work: tiles of 16 regions x 16 words per listed pair, three products per split element
            cx, cy = ci.to(torch.int64), cc.to(torch.int64)
            live = short >= 0
            c = short.clamp(min=0).to(torch.int64)
            q = torch.arange(short.shape[0], device=dev)[:, None].expand_as(short)
            rx, ty = (cx[q], cy[c]) if dim == 1 else (cx[c], cy[q])
            up = lambda v: (v + 15) // 16 * 16                                                               # noqa: E731
            nprod = 3 if args.precision == 'split' else 1
            tile_flop = int((2 * up(rx) * up(ty) * D * nprod)[live].sum())
            real_flop = int((2 * rx * ty * D * nprod)[live].sum())
            sec = r['rescore_kernel']['median_ms'] * 1e-3
            r['rescore_kernel'].update({'pairs': int(live.sum()), 'tile_flop': tile_flop, 'counted_flop': real_flop,
                                        'tile_tflops': round(tile_flop / sec / 1e12, 2),
                                        'share_of_fp16_peak': round(tile_flop / sec / PEAK_FP16_FLOPS, 4)})
            if with_grid:
                g, s = r['alignment_grid+topk_indices'], r['search_rerank']
                r['speedup_over_grid'] = round(g['median_ms'] / s['median_ms'], 2)
                r['difference_over_larger_spread'] = round((g['median_ms'] - s['median_ms']) / max(g['spread_ms'], s['spread_ms'], 1e-6), 2)
                full = grid()
                agree = (full[:, 0] == idx[:, 0]).float().mean().item()
                r['top1_equals_full_alignment_ranking'] = round(agree, 4)                 # the shortlist's recall of the grid's top-1
            top10 = min(10, k)
            same10 = torch.tensor([len(set(a) & set(b)) for a, b in zip(idx[:, :top10].tolist(), short[:, :top10].tolist())])
            r['quality_vs_shortlist'] = {'top1_differs': round((idx[:, 0] != short[:, 0]).float().mean().item(), 4),
                                         'top10_set_differs': round((same10 < top10).float().mean().item(), 4),
                                         'top10_mean_overlap': round(same10.float().mean().item() / top10, 4)}
            res['directions'][direction] = r
        out['sizes'][str(n_img)] = res
        del si, sc, x, y
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
