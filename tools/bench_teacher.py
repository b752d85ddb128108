#!/usr/bin/env python3
"""The cross-encoder teacher's attention window (ops.attention_window_mean, csrc/attn_window.hip) and teacher.get_teacher_scores.
Prints ONE JSON line (and writes it to --out).

(a) the kernel against the plain formulation in torch on the same GPU (plain_window below: matmul, add the mask, softmax,
    mean over heads, slice -- the reference's arithmetic for one layer): H 12, dh 64, L 140, rows 1:70, columns 70:140, at N = 40 (the
    reference's chunk) and N = 1024 (B = 32).  Per path the median per-call time and the peak of torch.cuda.max_memory_allocated
    above what was allocated before the call.
(b) get_teacher_scores end to end on a random-weight VinVL-base configuration at 64 sequences of 70 + 70 positions, subdivs 40: the
    fused window, fused=False (the last layer in torch ops), and the reference's dataflow (output_attentions=True: every layer keeps
    its probabilities; tests' bookkeeping restated inline).

Before timing, the paths must agree to 1e-6.  Protocol (tools/bench_xent.py): one process; a clock-settling pre-roll; then
`--rounds` rounds (>= 5) in which the paths alternate, each timed over its calls between two HIP events; per path the median of
the rounds' per-call times with min / max (max - min is the spread the summary condition uses).  There is no fallback: without an
MI355X this fails."""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, DH, L, ROWS, COLS, TEXT_LEN = 12, 64, 140, (1, 69), (70, 70), 70


def main():
    faulthandler.enable()
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=40)
    ap.add_argument('--preroll-s', type=float, default=1.0)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    from aladin_amd import backbone, ops, synth, teacher
    if not torch.cuda.is_available():
        raise SystemExit('bench_teacher: needs the MI355X (no GPU visible, no fallback)')
    dev = torch.device('cuda:0')

    def plain_window(q, k, add):
        qh = q.view(q.shape[0], L, H, DH).permute(0, 2, 1, 3)
        kh = k.view(k.shape[0], L, H, DH).permute(0, 2, 1, 3)
        probs = torch.softmax(torch.matmul(qh, kh.transpose(-1, -2)) / (DH ** 0.5) + add, dim=-1)
        return probs.mean(dim=1)[:, ROWS[0]:ROWS[0] + ROWS[1], COLS[0]:COLS[0] + COLS[1]]

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def peak_bytes(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    def measure(paths, calls):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.preroll_s:
            for fn in paths.values():
                fn()
            torch.cuda.synchronize()
        ms = {name: [] for name in paths}
        for _ in range(args.rounds):
            for name, fn in paths.items():
                ms[name].append(timed(fn, calls))
        return {name: {'median_ms': round(statistics.median(v), 5), 'min_ms': round(min(v), 5), 'max_ms': round(max(v), 5),
                       'peak_bytes': peak_bytes(paths[name])} for name, v in ms.items()}

    out = {'tool': 'bench_teacher', 'rounds': args.rounds, 'preroll_s': args.preroll_s, 'device': torch.cuda.get_device_name(0),
           'window': {'heads': H, 'dh': DH, 'L': L, 'rows': [ROWS[0], ROWS[0] + ROWS[1]], 'cols': [COLS[0], COLS[0] + COLS[1]]},
           'comparator': 'plain torch on the same GPU: matmul, add the -10000 mask, softmax, mean over heads, slice', 'kernel': {},
           'teacher': {}}
    with torch.no_grad():
        # ---- (a) the kernel
        for N in (40, 1024):
            gen = torch.Generator(device=dev).manual_seed(11)
            q = torch.randn((N, L, H * DH), device=dev, generator=gen)
            k = torch.randn((N, L, H * DH), device=dev, generator=gen)
            keep = torch.from_numpy(synth.integers((N, 2), 8, 70, 13)).to(dev)
            pos = torch.arange(70, device=dev)[None, :]
            mask = torch.cat([(pos < keep[:, :1]), (pos < keep[:, 1:])], 1).to(torch.int64)
            add = ((1.0 - mask.float()) * -10000.0)[:, None, None, :]
            res_buf = torch.empty((N, ROWS[1], COLS[1]), device=dev)
            paths = {'hip': lambda: ops.attention_window_mean(q, k, mask, H, ROWS, COLS, out=res_buf),
                     'torch': lambda: plain_window(q, k, add)}
            err = float((paths['hip']() - paths['torch']()).abs().max())
            assert err <= 1e-6, err
            calls = max(args.calls // (1 if N == 40 else 8), 3)
            res = measure(paths, calls)
            res['calls_per_round'] = calls
            res['max_abs_diff'] = err
            res['torch_over_hip'] = round(res['torch']['median_ms'] / res['hip']['median_ms'], 2)
            res['torch_spread_ms'] = round(res['torch']['max_ms'] - res['torch']['min_ms'], 5)
            res['hip_not_slower_than_torch_by_more_than_its_spread'] = bool(
                res['hip']['median_ms'] <= res['torch']['median_ms'] + res['torch_spread_ms'])
            out['kernel']['N%d' % N] = res
            del q, k, res_buf, paths
        torch.cuda.empty_cache()

        # ---- (b) the teacher end to end: VinVL base, random weights, 64 sequences of 70 + 70 positions
        n = 64
        torch.manual_seed(0)
        cfg = backbone.BertConfig()
        model = backbone.ImageBertForSequenceClassification(cfg).eval().to(dev)
        cfg_all = backbone.BertConfig(output_attentions=True)
        model_all = backbone.ImageBertForSequenceClassification(cfg_all).eval().to(dev)
        model_all.load_state_dict(model.state_dict())
        keep = synth.integers((n, 2), 8, 70, 23)
        pos = np.arange(70)[None, :]
        mask_np = np.concatenate([pos < keep[:, :1], pos < keep[:, 1:]], 1).astype(np.int64)
        ids = synth.integers((n, 70), 1, cfg.vocab_size - 1, 21) * mask_np[:, :70]
        batch = (torch.from_numpy(ids).to(dev), torch.from_numpy(mask_np).to(dev), torch.zeros((n, 70), dtype=torch.int64, device=dev),
                 torch.from_numpy(synth.normal((n, 70, cfg.img_feature_dim), 22) * mask_np[:, 70:, None].astype(np.float32)).to(dev),
                 torch.zeros(n, dtype=torch.int64, device=dev))
        a = types.SimpleNamespace(device=dev, num_labels=cfg.num_labels)

        def all_layers(subdivs=40):
            results, atts = [], []
            for b in range(0, n, subdivs):
                o = model_all(input_ids=batch[0][b:b + subdivs], attention_mask=batch[1][b:b + subdivs],
                              token_type_ids=batch[2][b:b + subdivs], img_feats=batch[3][b:b + subdivs])
                results.append(torch.softmax(o[0], dim=1)[:, 1])
                atts.append(o[1][-1].mean(dim=1)[:, 1:TEXT_LEN, TEXT_LEN:])
            return torch.cat(results).view(8, 8), torch.cat(atts).view(8, 8, TEXT_LEN - 1, L - TEXT_LEN)
        paths = {'fused': lambda: teacher.get_teacher_scores(a, model, batch, 40, fused=True),
                 'plain_last_layer': lambda: teacher.get_teacher_scores(a, model, batch, 40, fused=False),
                 'all_layers': all_layers}
        want = paths['all_layers']()
        for name in ('fused', 'plain_last_layer'):
            got = paths[name]()
            assert float((got[0] - want[0]).abs().max()) <= 1e-5 and float((got[1] - want[1]).abs().max()) <= 1e-6, name
        calls = max(args.calls // 8, 3)
        res = measure(paths, calls)
        res['calls_per_round'] = calls
        res['sequences'] = n
        res['subdivs'] = 40
        res['all_layers_over_fused'] = round(res['all_layers']['median_ms'] / res['fused']['median_ms'], 3)
        res['plain_last_layer_over_fused'] = round(res['plain_last_layer']['median_ms'] / res['fused']['median_ms'], 3)
        out['teacher'] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
