#!/usr/bin/env python3
"""The semantic contrastive loss (loss.SemanticContrastiveLoss -> ops.semantic_hinge_loss, csrc/semantic.hip), forward + backward
from the embeddings with measure 'dot', at (B, D) = (32, 768) -- the shipped batch size -- (256, 768) and (2048, 768), against the
reference's formulation in plain torch on the same GPU: per row and per column a nonzero() of the thresholded relevances, a host
randint and a mask write (2B device-to-host read-backs a step), boolean-mask gathers of the anchors, two clamped cost matrices,
autograd's backward.  Also ops.semantic_hinge_loss alone (a given score matrix, no products) at B = 2048.  Prints ONE JSON line.

The HIP path is timed eagerly (per-call launches, the host included) and as the replay of a captured HIP graph; the torch
formulation only eagerly: its nonzero() has a data-dependent shape and synchronises, so it cannot be captured.  Relevances: blocks of
five captions at 0.7 around a diagonal of 1 (COCO's five captions per image), threshold 0.4.  Before timing, the two must agree
where the choice is forced (identity relevances: one candidate per line): loss within rtol 1e-5, gradients equal within 1e-4 of
their largest entry.

Protocol (tools/bench_entropy.py): one process; a clock-settling pre-roll; then `--rounds` rounds (>= 5) in which the paths
alternate, each timed over its calls between two HIP events; per path the median of the rounds' per-call times with min / max.
There is no fallback: without an MI355X this fails."""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGIN, THRESHOLD = 0.2, 0.4


def main():
    faulthandler.enable()
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--preroll-s', type=float, default=1.0)
    args = ap.parse_args()
    import torch
    from aladin_amd import ops, synth
    from aladin_amd.loss import SemanticContrastiveLoss
    if not torch.cuda.is_available():
        raise SystemExit('bench_semantic: needs the MI355X (no GPU visible, no fallback)')
    dev = torch.device('cuda:0')

    def pick_one_per_line(match):
        """one True per row of `match`, drawn on the host among the row's True entries"""
        chosen = torch.zeros_like(match)
        for v in range(match.shape[0]):
            cand = match[v].nonzero()
            chosen[v, cand[torch.randint(cand.shape[0], (1,))]] = True
        return chosen

    def torch_scores_term(S, rel, max_violation):
        B = S.shape[0]
        match = rel > THRESHOLD
        a1 = S[pick_one_per_line(match)].view(B, 1)
        a2 = S[pick_one_per_line(match.t()).t()].view(1, B)          # read back row-major, as the reference does
        off = ~torch.eye(B, dtype=torch.bool, device=S.device)
        cs = (MARGIN + S - a1).clamp(min=0) * off
        ci = (MARGIN + S - a2).clamp(min=0) * off
        if max_violation:
            return cs.max(1)[0].sum() + ci.max(0)[0].sum()
        return cs.sum() + ci.sum()

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
        torch.testing.assert_close(got[0], want[0], rtol=1e-5, atol=0)
        for u, v in zip(got[1:], want[1:]):
            torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-4 * float(v.abs().max()))

    def measure(paths, calls):
        """paths: {name: (fn, calls per round)}"""
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.preroll_s:
            for name, (fn, _) in paths.items():
                if name != 'torch_eager':
                    fn()
            torch.cuda.synchronize()
        ms = {name: [] for name in paths}
        for _ in range(args.rounds):
            for name, (fn, n) in paths.items():
                ms[name].append(timed(fn, n))
        res = {name: summary(v) for name, v in ms.items()}
        res['calls_per_round'] = {name: n for name, (_, n) in paths.items()}
        res['torch_eager_over_hip_eager'] = round(res['torch_eager']['median_ms'] / res['hip_eager']['median_ms'], 2)
        res['torch_eager_over_hip_graph'] = round(res['torch_eager']['median_ms'] / res['hip_graph']['median_ms'], 2)
        return res

    def group_relevances(B):
        g = torch.arange(B, device=dev) // 5
        rel = torch.where(g[:, None] == g[None, :], 0.7, 0.0).to(torch.float32)
        rel.fill_diagonal_(1.0)
        return rel

    out = {'tool': 'bench_semantic', 'rounds': args.rounds, 'calls_per_round': args.calls, 'preroll_s': args.preroll_s,
           'device': torch.cuda.get_device_name(0), 'margin': MARGIN, 'threshold': THRESHOLD, 'max_violation': False,
           'relevances': 'blocks of 5 at 0.7, diagonal 1',
           'comparator': "the reference's formulation in plain torch on the same GPU, eager only (2B nonzero read-backs; not capturable)",
           'shapes': {}}
    for B, D in ((32, 768), (256, 768), (2048, 768)):
        img, cap = synth.global_embeddings(B, D, seed=8, noise=1.0)
        rel, eye = group_relevances(B), torch.eye(B, device=dev)
        draws = torch.randint(0, 2 ** 31 - 1, (2 * B,), dtype=torch.int32, device=dev)
        calls = args.calls if B < 2048 else max(args.calls // 4, 10)
        torch_calls = max(1, min(calls, 4096 // (2 * B)))               # the reference's loop costs ~2B read-backs a call

        # every path has leaves of its own, first used on the stream it runs on (tools/bench_xent.py)
        def leaves():
            return torch.from_numpy(img).to(dev).requires_grad_(True), torch.from_numpy(cap).to(dev).requires_grad_(True)

        def hip_step_of(relevances):
            a, b = leaves()
            crit = SemanticContrastiveLoss(margin=MARGIN, threshold=THRESHOLD, measure='dot')

            def step():
                loss = crit(a, b, relevances, draws=draws)
                return (loss.detach(),) + torch.autograd.grad(loss, (a, b))
            return step

        def torch_step_of(relevances):
            a, b = leaves()

            def step():
                loss = torch_scores_term(a @ b.t(), relevances, False)
                return (loss.detach(),) + torch.autograd.grad(loss, (a, b))
            return step
        agree(hip_step_of(eye)(), torch_step_of(eye)())
        got = hip_step_of(rel)()
        res = measure({'hip_eager': (hip_step_of(rel), calls), 'torch_eager': (torch_step_of(rel), torch_calls),
                       'hip_graph': (captured(hip_step_of(rel)).replay, calls)}, calls)
        res['loss'] = round(float(got[0]), 4)
        out['shapes']['%dx%d' % (B, D)] = res

    # the criterion alone on a given score matrix
    B = 2048
    img, cap = synth.global_embeddings(B, 768, seed=8, noise=1.0)
    S0 = torch.from_numpy(img).to(dev) @ torch.from_numpy(cap).to(dev).t()
    rel, eye = group_relevances(B), torch.eye(B, device=dev)
    draws = torch.randint(0, 2 ** 31 - 1, (2 * B,), dtype=torch.int32, device=dev)

    def scores_step_of(term):
        S = S0.clone().requires_grad_(True)

        def step():
            loss = term(S)
            return (loss.detach(),) + torch.autograd.grad(loss, (S,))
        return step
    hip = lambda relevances: (lambda S: ops.semantic_hinge_loss(S, relevances, MARGIN, THRESHOLD, draws=draws))      # noqa: E731
    ref = lambda relevances: (lambda S: torch_scores_term(S, relevances, False))                                     # noqa: E731
    agree(scores_step_of(hip(eye))(), scores_step_of(ref(eye))())
    calls = max(args.calls // 4, 10)
    out['scores_only_2048'] = measure({'hip_eager': (scores_step_of(hip(rel)), calls), 'torch_eager': (scores_step_of(ref(rel)), 1),
                                       'hip_graph': (captured(scores_step_of(hip(rel))).replay, calls)}, calls)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
