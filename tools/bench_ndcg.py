#!/usr/bin/env python3
"""nDCG evaluation (ops.ndcg_from_ranking, csrc/ndcg.hip) at COCO-5k scale: a 25000 x 5000 relevance matrix (captions x images),
rank = 25, both directions -- 't2i': the 25000 captions query 5000 images along the matrix rows; 'i2t': the 5000 images query
25000 captions along its COLUMNS (strided reads, reported separately).  Prints ONE JSON line.

Paths: the fused kernel (stages the row, selects the ideal DCG), the IDEAL_GIVEN path (the scorer's cached second call), and
evaluation.i2t / t2i end to end on a memoised 5000 x 25000 matching-head grid with and without a two-method DCG scorer.
The only comparator that exists is the reference's PROCEDURE -- one numpy argsort of the score row and one of the relevance row
per query and method, on one host core: it is timed here from the tests' numpy restatement (tests/helpers/ndcg_numpy.py) over a
sample of queries and SCALED to all queries and two methods; it is labelled as such in the output and reads nothing of the
reference.

Protocol (tools/bench_search.py): one process; a clock-settling pre-roll; then `--rounds` rounds (>= 5) in which the paths
alternate, each timed over `--calls` calls (>= 20) between two HIP events; per path the median of the rounds' per-call times
with min / max.  There is no fallback: without an MI355X this fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--preroll-s', type=float, default=1.0)
    ap.add_argument('--n-img', type=int, default=5000)
    ap.add_argument('--rank', type=int, default=25)
    ap.add_argument('--D', type=int, default=64)
    ap.add_argument('--host-sample', type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ndcg_numpy as N
    from aladin_amd import dcg, ops, synth
    from aladin_amd import evaluation as E
    if not torch.cuda.is_available():
        raise SystemExit('bench_ndcg: needs the MI355X (no GPU visible, no fallback)')
    dev = torch.device('cuda:0')
    n_img, n_cap, rank = args.n_img, 5 * args.n_img, args.rank

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

    def alternate(paths, calls):
        preroll(list(paths.values()))
        ms = {name: [] for name in paths}
        for _ in range(args.rounds):
            for name, fn in paths.items():
                ms[name].append(timed(fn, calls))
        return {name: summary(v) for name, v in ms.items()}

    gen = torch.Generator(device=dev).manual_seed(1407)
    rels = []
    for sparse in (False, True):                                            # 'rougeL'-like dense, 'spice'-like mostly zero
        r = 0.6 * torch.rand((n_cap, n_img), generator=gen, device=dev)
        if sparse:
            r = torch.where(torch.rand((n_cap, n_img), generator=gen, device=dev) < 0.7, torch.zeros_like(r), torch.round(r * 50) / 50)
        r[torch.arange(n_cap, device=dev), torch.arange(n_cap, device=dev) // 5] = 1.0
        rels.append(r)
    out = {'tool': 'bench_ndcg', 'relevance_shape': [n_cap, n_img], 'rank': rank, 'rounds': args.rounds, 'calls_per_round': args.calls,
           'preroll_s': args.preroll_s, 'device': torch.cuda.get_device_name(0), 'kernel': {}, 'end_to_end': {}}
    rel = rels[0]
    host = {}
    for direction, dim, n_q, n_c in (('t2i', 1, n_cap, n_img), ('i2t', 0, n_img, n_cap)):
        table = torch.randint(0, n_c, (n_q, rank), generator=gen, device=dev, dtype=torch.int32)
        nd, dc, ideal = ops.ndcg_from_ranking(rel, table, dim=dim, return_parts=True)
        given = ops.ndcg_from_ranking(rel, table, dim=dim, ideal=ideal, return_parts=True)
        assert torch.equal(given[0].view(torch.int64), nd.view(torch.int64)), 'the two paths disagree'
        res = alternate({'fused': lambda: ops.ndcg_from_ranking(rel, table, dim=dim, return_parts=True),
                         'ideal_given': lambda: ops.ndcg_from_ranking(rel, table, dim=dim, ideal=ideal)}, args.calls)
        res['queries'], res['gallery'] = n_q, n_c
        res['read'] = 'rows (contiguous)' if dim == 1 else 'columns (stride %d floats)' % n_img
        res['fused']['relevance_GBps'] = round(n_q * n_c * 4 / res['fused']['median_ms'] / 1e6, 1)
        out['kernel'][direction] = res
        # the reference's procedure on the host, sampled and scaled: per query one argsort of a score row + dcg.py:194-216
        sample = np.random.RandomState(3).choice(n_q, min(args.host_sample, n_q), replace=False)
        rows = (rel[sample] if dim == 1 else rel[:, sample].t()).cpu().numpy()
        scores = np.random.RandomState(4).random_sample(rows.shape).astype(np.float32)
        t0 = time.perf_counter()
        got = [N.ndcg_parts(rows[i], np.argsort(scores[i])[::-1][:rank])[0] for i in range(len(sample))]
        per_query = (time.perf_counter() - t0) / len(sample)
        err = float(np.abs(np.array(got) - ops.ndcg_from_ranking(
            torch.from_numpy(rows).to(dev), torch.from_numpy(np.ascontiguousarray(np.argsort(scores, axis=1)[:, ::-1][:, :rank]).astype(np.int32)).to(dev)
        ).cpu().numpy()).max())
        host[direction] = {'label': 'reference PROCEDURE (two numpy argsorts per query and method) timed from the numpy restatement on one '
                                    'host core over %d sampled queries and SCALED to %d queries x 2 methods; not the reference itself'
                                    % (len(sample), n_q),
                           'per_query_ms': round(1e3 * per_query, 4), 'scaled_two_methods_ms': round(1e3 * per_query * n_q * 2, 1),
                           'max_abs_difference_to_device_on_sample': err}
    out['host_procedure_scaled'] = host
    # end to end: i2t / t2i on a memoised matching-head grid, with and without a two-method scorer (second and later calls: the scorer
    # holds its windows and ideal DCGs, as in a validation loop)
    img_rows, cap_rows = synth.retrieval_embeddings(n_img, args.D, sigma=8.0)
    images = torch.from_numpy(img_rows).to(dev).unsqueeze(1)
    captions = torch.from_numpy(cap_rows).to(dev).unsqueeze(1)
    scorer = dcg.DCG(None, n_cap, 'test', rank=rank, relevance_methods=['rougeL', 'spice'], relevances=rels)
    e2e_calls = max(2, args.calls // 5)
    for name, fn in (('i2t', E.i2t), ('t2i', E.t2i)):
        t0 = time.perf_counter()
        first = fn(images, captions, None, None, ndcg_scorer=scorer)
        torch.cuda.synchronize()
        first_ms = 1e3 * (time.perf_counter() - t0)
        res = alternate({'without_scorer': lambda: fn(images, captions, None, None),
                         'with_scorer': lambda: fn(images, captions, None, None, ndcg_scorer=scorer)}, e2e_calls)
        res['calls_per_round'] = e2e_calls
        res['first_call_with_scorer_wall_ms'] = round(first_ms, 1)
        res['mean_ndcg'] = [round(float(v), 6) for v in first[5:]]
        res['added_by_scorer_ms'] = round(res['with_scorer']['median_ms'] - res['without_scorer']['median_ms'], 4)
        out['end_to_end'][name] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
