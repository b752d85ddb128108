#!/usr/bin/env python3
"""The attention-distillation loss (loss.AttentionDistillationLoss -> ops.attention_distillation_loss, csrc/attdistill.hip), forward +
backward from the sets, at the shipped shape -- B = 32, R = 51, T = 38, D = 768, teacher 32 x 32 x 69 x 70 -- and at B = 64, against
the reference's formulation in plain torch on the same GPU: expand + matmul into the (B, B, T', R') logits, masked log-softmax over
regions, F.normalize of the sliced teacher, the KL terms with the masked ones dropped (so that it is finite on ragged images),
autograd's backward.  Also the library alone at B = 256 (the torch formulation would hold 4 tensors of 1.2e8 floats there).
Prints ONE JSON line.

Both are timed eagerly (per-call launches, the host included: what a train loop without graphs pays) and as the replay of a
captured HIP graph (the device's share).  Before timing, the two must agree: loss within rtol 1e-5, gradients within rtol 1e-4 and
1e-5 of their largest entry.

Protocol (tools/bench_xent.py): one process; a clock-settling pre-roll; then `--rounds` rounds (>= 5) in which the paths
alternate, each timed over `--calls` calls between two HIP events; per path the median of the rounds' per-call times with
min / max.  There is no fallback: without an MI355X this fails."""
import argparse
import faulthandler
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, T, D, WT, RT = 51, 38, 768, 69, 70


def main():
    faulthandler.enable()
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--preroll-s', type=float, default=1.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from aladin_amd import synth
    from aladin_amd.loss import AttentionDistillationLoss
    if not torch.cuda.is_available():
        raise SystemExit('bench_attdistill: needs the MI355X (no GPU visible, no fallback)')
    dev = torch.device('cuda:0')

    def torch_term(im, s, rmask, wmask, n_rows, teacher):
        x, y = im[:, 1:, :], s[:, 1:, :]
        Bi, Bc = x.shape[0], y.shape[0]
        xe = x.unsqueeze(1).expand(-1, Bc, -1, -1)
        ye = y.unsqueeze(0).expand(Bi, -1, -1, -1)
        L = torch.matmul(ye, xe.transpose(2, 3)) / math.sqrt(x.shape[2])                 # (Bi, Bc, T', R')
        logp = torch.log_softmax(L.masked_fill(~rmask, float('-inf')), dim=-1)
        P = F.normalize(teacher[:, :, :y.shape[1], :x.shape[1]], p=1, dim=3)
        keep = rmask & wmask
        terms = torch.where(keep, torch.xlogy(P, P) - P * logp.masked_fill(~rmask, 0.0), torch.zeros((), device=L.device))
        return terms.sum() / n_rows

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
        if 'torch_eager' in res:
            res['torch_over_hip_eager'] = round(res['torch_eager']['median_ms'] / res['hip_eager']['median_ms'], 2)
            res['torch_over_hip_graph'] = round(res['torch_graph']['median_ms'] / res['hip_graph']['median_ms'], 2)
        return res

    out = {'tool': 'bench_attdistill', 'rounds': args.rounds, 'calls_per_round': args.calls, 'preroll_s': args.preroll_s,
           'device': torch.cuda.get_device_name(0), 'R': R, 'T': T, 'D': D, 'teacher': [WT, RT],
           'comparator': "the reference's formulation in plain torch on the same GPU (expand + matmul, masked log_softmax, F.normalize, "
                         'KL terms with the masked ones dropped, autograd)', 'shapes': {}}
    for B in (32, 64, 256):
        im_np, s_np, im_len, s_len = synth.alignment_batch(B, R, T, D, seed=5, ragged=True)
        teacher = torch.from_numpy((synth.uniform((B, B, WT, RT), 6) ** 4).astype(np.float32)).to(dev)
        n = torch.tensor(im_len, device=dev).clamp(max=R) - 1
        m = torch.tensor(s_len, device=dev).clamp(max=T) - 1
        rmask = (torch.arange(R - 1, device=dev)[None, :] < n[:, None])[:, None, None, :]
        wmask = (torch.arange(T - 1, device=dev)[None, :] < m[:, None])[None, :, :, None]
        n_rows = float(B * int(m.sum()))
        calls = max(args.calls // (1 if B == 32 else 4 if B == 64 else 20), 5)

        # every path has leaves of its own, first used on the stream it runs on, and nothing of an autograd graph outlives a step
        def leaves():
            return torch.from_numpy(im_np).to(dev).requires_grad_(True), torch.from_numpy(s_np).to(dev).requires_grad_(True)

        def hip_step_of():
            a, b = leaves()
            crit = AttentionDistillationLoss()

            def step():
                loss = crit(a, b, im_len, s_len, teacher)
                return (loss.detach(),) + torch.autograd.grad(loss, (a, b))
            return step

        def torch_step_of():
            a, b = leaves()

            def step():
                loss = torch_term(a, b, rmask, wmask, n_rows, teacher)
                return (loss.detach(),) + torch.autograd.grad(loss, (a, b))
            return step
        got = hip_step_of()()
        if B <= 64:
            want = torch_step_of()()
            torch.testing.assert_close(got[0], want[0], rtol=1e-5, atol=0)
            for u, v in zip(got[1:], want[1:]):
                torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-5 * float(v.abs().max()))
            res = measure({'hip_eager': hip_step_of(), 'torch_eager': torch_step_of()},
                          {'hip_graph': captured(hip_step_of()), 'torch_graph': captured(torch_step_of())}, calls)
        else:
            res = measure({'hip_eager': hip_step_of()}, {'hip_graph': captured(hip_step_of())}, calls)
        res['loss'] = round(float(got[0]), 6)
        res['calls_per_round'] = calls
        out['shapes']['B%d' % B] = res
        del teacher
    print(json.dumps(out))


if __name__ == '__main__':
    main()
