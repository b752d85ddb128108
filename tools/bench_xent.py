#!/usr/bin/env python3
"""The cross-entropy (InfoNCE) criterion (loss.CrossEntropyCriterion -> ops.match_cross_entropy, csrc/xent.hip), forward + backward
from the embeddings, at (B, D) = (32, 768) -- the shipped batch size -- (256, 768) and (2048, 768), against the same loss written
in plain torch on the same GPU: mm, exp of the temperature, logsumexp along both axes, the two diagonals, autograd's backward.
Also ops.cross_entropy_scores alone (a given score matrix, no products) at B = 2048.  Prints ONE JSON line.

Both are timed eagerly (per-call launches, the host included: what a train loop without graphs pays) and as the replay of a
captured HIP graph (the device's share).  Before timing, the two must agree: loss and d temperature within rtol 1e-5 / atol 1e-6,
gradients within rtol 1e-4 and 1e-5 of their largest entry.

Protocol (tools/bench_entropy.py): one process; a clock-settling pre-roll; then `--rounds` rounds (>= 5) in which the paths
alternate, each timed over `--calls` calls between two HIP events; per path the median of the rounds' per-call times with
min / max.  There is no fallback: without an MI355X this fails."""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    faulthandler.enable()
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--preroll-s', type=float, default=1.0)
    args = ap.parse_args()
    import torch
    from aladin_amd import ops, synth
    from aladin_amd.loss import CrossEntropyCriterion
    if not torch.cuda.is_available():
        raise SystemExit('bench_xent: needs the MI355X (no GPU visible, no fallback)')
    dev = torch.device('cuda:0')
    T0 = 2.0                                            # log-temperature of the timed runs (e^2 ~ 7.4); the time does not depend on it

    def torch_scores_term(S, t):
        # loss = 1/(2B) [ sum_i (LSE_j L_ij - L_ii) + sum_j (LSE_i L_ij - L_jj) ],  L = S e^t
        L = S * torch.exp(t)
        d = L.diagonal()
        return 0.5 * ((torch.logsumexp(L, 1) - d).mean() + (torch.logsumexp(L, 0) - d).mean())

    def torch_term(a, b, t):
        return torch_scores_term(a @ b.t(), t)

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def summary(ms):
        return {'median_ms': round(statistics.median(ms), 5), 'min_ms': round(min(ms), 5), 'max_ms': round(max(ms), 5)}

    def captured(step):
        cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        cur.wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        return graph

    def agree(got, want):
        torch.testing.assert_close(got[0], want[0], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(got[-1], want[-1], rtol=1e-5, atol=1e-6)
        for u, v in zip(got[1:-1], want[1:-1]):
            torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-5 * float(v.abs().max()))

    def measure(paths, graphs, calls):
        paths = dict(paths)
        paths.update({k: g.replay for k, g in graphs.items()})
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.preroll_s:
            for fn in paths.values():
                fn()
            torch.cuda.synchronize()
        ms = {name: [] for name in paths}
        for _ in range(args.rounds):
            for name, fn in paths.items():
                ms[name].append(timed(fn, calls))
        res = {name: summary(v) for name, v in ms.items()}
        res['torch_over_hip_eager'] = round(res['torch_eager']['median_ms'] / res['hip_eager']['median_ms'], 2)
        res['torch_over_hip_graph'] = round(res['torch_graph']['median_ms'] / res['hip_graph']['median_ms'], 2)
        return res

    out = {'tool': 'bench_xent', 'rounds': args.rounds, 'calls_per_round': args.calls, 'preroll_s': args.preroll_s,
           'device': torch.cuda.get_device_name(0), 'log_temperature': T0,
           'comparator': 'the same loss in plain torch on the same GPU (mm, logsumexp along both axes, autograd)', 'shapes': {}}
    for B, D in ((32, 768), (256, 768), (2048, 768)):
        img, cap = synth.global_embeddings(B, D, seed=8, noise=1.0)
        calls = args.calls if B < 2048 else max(args.calls // 4, 10)

        # Every path has leaves of its own, first used on the stream it runs on, and nothing of an autograd graph outlives a step
        # (tools/bench_entropy.py: a backward inside a capture must not meet a gradient accumulator made on another stream).
        def leaves():
            return (torch.from_numpy(img).to(dev).requires_grad_(True), torch.from_numpy(cap).to(dev).requires_grad_(True),
                    torch.full((1,), T0, device=dev, requires_grad=True))

        def hip_step_of():
            a, b, _ = leaves()
            crit = CrossEntropyCriterion().to(dev)
            with torch.no_grad():
                crit.temperature.fill_(T0)

            def step():
                loss = crit(a, b)
                return (loss.detach(),) + torch.autograd.grad(loss, (a, b, crit.temperature))
            return step

        def torch_step_of():
            a, b, t = leaves()

            def step():
                loss = torch_term(a, b, t)
                return (loss.detach(),) + torch.autograd.grad(loss, (a, b, t))
            return step
        got, want = hip_step_of()(), torch_step_of()()
        agree(got, want)
        res = measure({'hip_eager': hip_step_of(), 'torch_eager': torch_step_of()},
                      {'hip_graph': captured(hip_step_of()), 'torch_graph': captured(torch_step_of())}, calls)
        res['loss'] = round(float(got[0]), 6)
        out['shapes']['%dx%d' % (B, D)] = res

    # the criterion alone on a given score matrix
    B = 2048
    img, cap = synth.global_embeddings(B, 768, seed=8, noise=1.0)
    S0 = torch.from_numpy(img).to(dev) @ torch.from_numpy(cap).to(dev).t()

    def scores_step_of(term):
        S, t = S0.clone().requires_grad_(True), torch.full((1,), T0, device=dev, requires_grad=True)

        def step():
            loss = term(S, t)
            return (loss.detach(),) + torch.autograd.grad(loss, (S, t))
        return step
    agree(scores_step_of(ops.cross_entropy_scores)(), scores_step_of(torch_scores_term)())
    out['scores_only_2048'] = measure({'hip_eager': scores_step_of(ops.cross_entropy_scores), 'torch_eager': scores_step_of(torch_scores_term)},
                                      {'hip_graph': captured(scores_step_of(ops.cross_entropy_scores)),
                                       'torch_graph': captured(scores_step_of(torch_scores_term))}, max(args.calls // 4, 10))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
