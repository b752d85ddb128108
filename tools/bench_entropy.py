#!/usr/bin/env python3
"""The 'entropy' loss term (ops.nn_entropy_loss, csrc/entropy.hip), forward + backward, at (B, D) = (32, 768) -- the shipped batch
size -- and (256, 768), against the reference's formulation (alad/alad_model.py:17-27, 410-421) written in plain torch and run on
the same GPU: cat, mm, diagonal fill, max, gather, pairwise distance, log, mean and autograd's backward.  Prints ONE JSON line.

Both are timed eagerly (per-call launches, the host included: what a train loop without graphs pays) and as the replay of a
captured HIP graph (the device's share).  Before timing, the two must agree: same neighbours, loss within rtol 1e-5, gradients
within rtol 1e-4 / atol 1e-6.

Protocol (tools/bench_search.py): one process; a clock-settling pre-roll; then `--rounds` rounds (>= 5) in which the paths
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
    import torch.nn.functional as F
    from aladin_amd import ops, synth
    if not torch.cuda.is_available():
        raise SystemExit('bench_entropy: needs the MI355X (no GPU visible, no fallback)')
    dev = torch.device('cuda:0')

    def torch_term(a, b):
        x = torch.cat([a, b], 0)
        n = x.shape[0]
        dots = x @ x.t()
        dots.diagonal().fill_(-1)
        nn = dots.max(1).indices
        return -(n * F.pairwise_distance(x, x[nn])).log().mean(), nn

    def hip_term(a, b, neighbours=False):             # timed as the model calls it: the int64 copy of the neighbours is not asked for
        return ops.nn_entropy_loss(a, b, return_neighbours=True) if neighbours else (ops.nn_entropy_loss(a, b), None)

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

    out = {'tool': 'bench_entropy', 'rounds': args.rounds, 'calls_per_round': args.calls, 'preroll_s': args.preroll_s,
           'device': torch.cuda.get_device_name(0), 'comparator': "the reference's formulation in plain torch on the same GPU", 'shapes': {}}
    for B, D in ((32, 768), (256, 768)):
        img, cap = synth.global_embeddings(B, D, seed=8, noise=1.0)

        def leaves():
            return torch.from_numpy(img).to(dev).requires_grad_(True), torch.from_numpy(cap).to(dev).requires_grad_(True)

        def check():
            a, b = leaves()
            got, want = {}, {}
            for term, res in ((hip_term, got), (torch_term, want)):
                loss, res['nn'] = term(a, b, True) if term is hip_term else term(a, b)
                res['loss'] = loss.detach()
                res['d_img'], res['d_cap'] = torch.autograd.grad(loss, (a, b))
            assert torch.equal(got['nn'], want['nn']), 'the neighbours differ'
            torch.testing.assert_close(got['loss'], want['loss'], rtol=1e-5, atol=1e-6)
            for k in ('d_img', 'd_cap'):
                torch.testing.assert_close(got[k], want[k], rtol=1e-4, atol=1e-6)
            return float(got['loss'])
        loss_value = check()

        # Every path has leaves of its own, first used on the stream it runs on, and nothing of an autograd graph outlives a step:
        # a leaf's gradient accumulator remembers the stream it was made on, and a backward inside a capture that meets one made on
        # the default stream makes that stream wait for the capturing one, which ends the capture (and crashed the process here).
        def step_of(term):
            a, b = leaves()

            def step():
                loss, _ = term(a, b)
                torch.autograd.grad(loss, (a, b))
            return step
        paths = {'hip_eager': step_of(hip_term), 'torch_eager': step_of(torch_term)}
        graphs = {'hip_graph': captured(step_of(hip_term)), 'torch_graph': captured(step_of(torch_term))}
        paths.update({k: g.replay for k, g in graphs.items()})
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.preroll_s:
            for fn in paths.values():
                fn()
            torch.cuda.synchronize()
        ms = {name: [] for name in paths}
        for _ in range(args.rounds):
            for name, fn in paths.items():
                ms[name].append(timed(fn, args.calls))
        res = {name: summary(v) for name, v in ms.items()}
        res['torch_over_hip_eager'] = round(res['torch_eager']['median_ms'] / res['hip_eager']['median_ms'], 2)
        res['torch_over_hip_graph'] = round(res['torch_graph']['median_ms'] / res['hip_graph']['median_ms'], 2)
        res['loss'] = round(loss_value, 6)
        out['shapes']['%dx%d' % (B, D)] = res
        del graphs
    print(json.dumps(out))


if __name__ == '__main__':
    main()
