#!/usr/bin/env python3
"""ROUGE-L relevance (ops.rouge_l_relevance, csrc/rouge.hip) at COCO-5k scale: 25000 synthetic captions (5 per image, 8..20 tokens,
mean about 10.5, Zipf-distributed ids over about 8000 words) scored against the 5000 images they belong to -- the 25000 x 5000
float32 matrix of alad/evaluate_utils/compute_relevance.py.  Prints ONE JSON line.

Paths: the full matrix in one call (device time), and rouge.write_relevance_file end to end (tokenizing the caption strings,
uploading, the kernel in query-row chunks, the copies back and the file; wall time).
The only comparator that exists is the reference's PROCEDURE -- one plain LCS table per (query, reference caption) pair and the
F-measure, on one host core: it is timed here from the tests' numpy restatement of the plain dynamic programme
(tests/helpers/rouge_numpy.py: lcs_dp) over a sample of (query, image) pairs and SCALED to the whole matrix; it is labelled as such in
the output and reads nothing of the reference.  The sample's device values must equal the restatement's bit for bit.

Protocol (tools/bench_ndcg.py): one process; a clock-settling pre-roll; then `--rounds` rounds (>= 5), each timed over `--calls`
calls between two HIP events; the median of the rounds' per-call times with min / max.  There is no fallback: without an MI355X
this fails."""
import argparse
import json
import os
import statistics
import sys
import tempfile
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
    ap.add_argument('--vocab', type=int, default=8000)
    ap.add_argument('--host-sample', type=int, default=2000)
    ap.add_argument('--file-rounds', type=int, default=3)
    ap.add_argument('--fixed-len', type=int, default=0,
                    help='every caption this long (the same number of steps without the wait for a wave\'s longest reference)')
    args = ap.parse_args()
    import numpy as np
    import torch
    import rouge_numpy as R
    from aladin_amd import ops, rouge
    if not torch.cuda.is_available():
        raise SystemExit('bench_rouge: needs the MI355X (no GPU visible, no fallback)')
    dev = torch.device('cuda:0')
    n_img, n_cap = args.n_img, 5 * args.n_img
    rng = np.random.RandomState(1407)
    lens = np.clip(rng.poisson(2.5, size=n_cap) + 8, 8, 20)
    if args.fixed_len > 0:
        lens[:] = args.fixed_len
    ids = [np.minimum(rng.zipf(1.2, size=int(n)), args.vocab) - 1 for n in lens]
    captions = [' '.join('w%d' % v for v in row) for row in ids]
    tok, off, vocab = rouge.tokenize(captions)
    tok_d, off_d = torch.from_numpy(tok).to(dev), torch.from_numpy(off).to(dev)
    grp_d = torch.arange(0, n_cap + 1, 5, dtype=torch.int64, device=dev)
    out = torch.empty((n_cap, n_img), dtype=torch.float32, device=dev)
    steps = n_cap * int(lens.sum())                                         # (query, gallery token) pairs: the LCS update steps

    def full():
        ops.rouge_l_launch(tok_d, off_d, int(lens.max()), tok_d, off_d, int(lens.max()), grp_d, out)

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.preroll_s:
        full()
        torch.cuda.synchronize()
    ms = [timed(full, args.calls) for _ in range(args.rounds)]
    med = statistics.median(ms)
    res = {'tool': 'bench_rouge', 'captions': n_cap, 'images': n_img, 'caps_per_img': 5, 'mean_len': round(float(lens.mean()), 3),
           'max_len': int(lens.max()), 'distinct_words': len(vocab), 'rounds': args.rounds, 'calls_per_round': args.calls,
           'preroll_s': args.preroll_s, 'device': torch.cuda.get_device_name(0),
           'full_matrix': {'median_ms': round(med, 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3),
                           'spread_ms': round(max(ms) - min(ms), 3), 'scores_per_s': round(n_cap * n_img / med * 1e3, 1),
                           'pair_token_steps': steps, 'pair_token_steps_per_s': round(steps / med * 1e3, 1)}}
    own = out[torch.arange(n_cap, device=dev), torch.arange(n_cap, device=dev) // 5]
    assert bool((own == 1.0).all()), 'a caption against its own image must score exactly 1.0'
    res['full_matrix']['zero_fraction'] = round(float((out == 0).float().mean()), 4)

    # the reference's procedure on the host, sampled and scaled: per (query, image) five plain LCS tables and the F-measure
    srng = np.random.RandomState(3)
    qs, js = srng.randint(0, n_cap, size=args.host_sample), srng.randint(0, n_img, size=args.host_sample)
    seqs = [list(row) for row in ids]
    t0 = time.perf_counter()
    host = np.array([R.score(seqs[q], seqs[5 * j:5 * j + 5], R.lcs_dp) for q, j in zip(qs, js)], dtype=np.float32)
    per_score = (time.perf_counter() - t0) / len(qs)
    got = out[torch.from_numpy(qs).to(dev), torch.from_numpy(js).to(dev)].cpu().numpy()
    res['host_procedure_scaled'] = {
        'label': 'reference PROCEDURE (five plain LCS tables and the F-measure per score) timed from the numpy restatement on one host '
                 'core over %d sampled (query, image) pairs and SCALED to %d scores; not the reference itself' % (len(qs), n_cap * n_img),
        'per_score_us': round(1e6 * per_score, 2), 'scores_per_s': round(1.0 / per_score, 1),
        'scaled_core_hours': round(per_score * n_cap * n_img / 3600.0, 2),
        'sample_bits_differing_from_device': int((host.view(np.uint32) != got.view(np.uint32)).sum())}
    assert res['host_procedure_scaled']['sample_bits_differing_from_device'] == 0, 'the device disagrees with the restatement'

    # end to end: strings in, the relevance file out
    walls = []
    with tempfile.TemporaryDirectory() as tmp:
        config = {'dataset': {'data': tmp, 'name': 'bench'}}
        for _ in range(args.file_rounds):
            t0 = time.perf_counter()
            path = rouge.write_relevance_file(config, 'test', captions)
            walls.append(1e3 * (time.perf_counter() - t0))
        size = os.path.getsize(path)
        back = np.fromfile(path, dtype=np.float32, count=5 * n_img)
    assert size == 4 * n_cap * n_img and np.array_equal(back.view(np.uint32), out[:5].cpu().numpy().reshape(-1).view(np.uint32))
    res['write_relevance_file'] = {'chunk_rows': 4096, 'file_MB': round(size / 1e6, 1), 'median_wall_ms': round(statistics.median(walls), 1),
                                   'min_wall_ms': round(min(walls), 1), 'max_wall_ms': round(max(walls), 1), 'rounds': args.file_rounds}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
