#!/usr/bin/env python3
"""Whole library builds against a yardstick build on ONE box, per score-kernel body: five alternations, every run a fresh child
process with ALADIN_LIB set (see tools/ab_bench.py, which this runs as it is for the headline rows).

    python tools/ab_epilogues.py run OUT.json parent=aladin_amd/lib/old.so branch=aladin_amd/lib/libaladin_hip.so [more=...]
    python tools/ab_epilogues.py child          (one timing pass of the library ALADIN_LIB selects, a JSON line on stdout)

Rows: the headline step and score kernel; 200 event-timed ops.alignment_scores calls after 30 of warm-up for each shape of
SCORE_ROWS at D = 768; the sum-of-violations step with the dense arg-max table forced at B = 256 for ARGMAX_ROWS.  A build passes a
row when its median is at most the yardstick's (the first library's) median plus the yardstick's own max - min."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCORE_ROWS = [(256, 256, 51, 38), (254, 270, 51, 38), (256, 256, 60, 50), (256, 256, 34, 67), (32, 32, 34, 50), (32, 32, 51, 38), (64, 64, 71, 71)]
ARGMAX_ROWS = [(34, 50), (51, 38), (49, 38)]      # (49, 38): no side rows
D = 768


def batch(torch, np, Bi, Bc, R, Tn, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    im = torch.randn(Bi, R, D, device='cuda', generator=g)
    s = torch.randn(Bc, Tn, D, device='cuda', generator=g)
    rs = np.random.RandomState(seed)
    il, sl = list(rs.randint(10, R + 1, Bi)), list(rs.randint(6, Tn + 1, Bc))
    il[0], sl[0] = R, Tn
    return im, s, [int(x) for x in il], [int(x) for x in sl]


def child():
    import numpy as np
    import torch
    from aladin_amd import ops
    from aladin_amd.loss import AlignmentContrastiveLoss
    out = {}

    def timed(fn, iters, warm):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for (Bi, Bc, R, Tn) in SCORE_ROWS:
        im, s, il, sl = batch(torch, np, Bi, Bc, R, Tn, 31 * R + Tn)
        with torch.no_grad():
            out['scores %dx%d R%d T%d' % (Bi, Bc, R, Tn)] = timed(lambda: ops.alignment_scores(im, s, il, sl), 200, 30)
    crit = AlignmentContrastiveLoss(margin=0.2, measure='dot', max_violation=False, aggregation='MrSw')
    ops.DENSE_BACKWARD, ops.DENSE_ROWS_GEMM, ops.DENSE_MIN_FRACTION, ops.DENSE_GEMM_FORCE = True, True, 0.0, True
    for (R, Tn) in ARGMAX_ROWS:
        im, s, il, sl = batch(torch, np, 256, 256, R, Tn, 77 * R + Tn)
        a, b = im.requires_grad_(True), s.requires_grad_(True)

        def step():
            a.grad = None
            b.grad = None
            crit(a, b, il, sl).backward()
        out['sum-of-violations step 256 R%d T%d' % (R, Tn)] = timed(step, 50, 10)
        assert ops._LAST_BWD_FLAGS[0] & 2, 'the dense path was not taken'
    print('RESULT ' + json.dumps(out), flush=True)


def run(out_path, *lib_args):
    libs = [(a.split('=', 1)[0], os.path.abspath(a.split('=', 1)[1])) for a in lib_args]
    raw = {n: {} for n, _ in libs}
    # headline: tools/ab_bench.py as it is
    cmd = ['timeout', '-k', '10', '800', sys.executable, os.path.join(ROOT, 'tools', 'ab_bench.py'), '--reps', '5']
    for n, path in libs:
        cmd += ['--lib', n + '=' + path]
    p = subprocess.run(cmd, capture_output=True, text=True)
    print(p.stdout, p.stderr[-2000:], flush=True)
    if p.returncode != 0 or 'FAILED' in p.stdout:
        sys.exit('ab_bench failed with %d: nothing more is started' % p.returncode)
    for l in p.stdout.splitlines():
        w = l.split()
        if len(w) >= 10 and w[1] == 'step' and w[0] in raw:
            raw[w[0]].setdefault('headline step ms', []).append(float(w[2]))
            raw[w[0]].setdefault('headline score kernel us', []).append(float(w[6]))
            raw[w[0]].setdefault('headline loss', []).append(float(w[9]))
    for rep in range(5):
        for name, path in libs:
            c = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.abspath(__file__), 'child'], env=dict(os.environ, ALADIN_LIB=path),
                               capture_output=True, text=True)
            line = [l for l in c.stdout.splitlines() if l.startswith('RESULT ')]
            if c.returncode != 0 or not line:
                print(c.stdout[-2000:], c.stderr[-3000:])
                sys.exit('%s child failed with %d: nothing more is started' % (name, c.returncode))
            for k, v in json.loads(line[0][7:]).items():
                raw[name].setdefault(k + ' ms', []).append(v)
            print(rep, name, 'ok', flush=True)
    med = lambda x: sorted(x)[len(x) // 2]
    base = libs[0][0]
    rows, ok = {}, {n: True for n, _ in libs[1:]}
    for k in raw[base]:
        if k == 'headline loss':
            continue
        pa = raw[base][k]
        rows[k] = {base + '_median': med(pa), base + '_spread': max(pa) - min(pa)}
        txt = '%-44s %s %.4f (spread %.4f)' % (k, base, med(pa), max(pa) - min(pa))
        for n, _ in libs[1:]:
            good = med(raw[n][k]) <= med(pa) + (max(pa) - min(pa))
            rows[k][n + '_median'], rows[k][n + '_pass'] = med(raw[n][k]), good
            ok[n] &= good
            txt += '  %s %.4f %s' % (n, med(raw[n][k]), 'pass' if good else 'FAIL')
        print(txt)
    json.dump({'rule': 'median <= yardstick median + (yardstick max - yardstick min), five alternations in one session', 'yardstick': base,
               'raw': raw, 'rows': rows, 'all_pass': ok}, open(out_path, 'w'), indent=1)


if __name__ == '__main__':
    if sys.argv[1] == 'child':
        child()
    else:
        run(*sys.argv[2:])
