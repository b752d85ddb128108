"""Generate tests/golden/entropy.npz and tests/golden/signatures_entropy.json by running the REFERENCE (mesnico/ALADIN) 'entropy' loss
term: alad/alad_model.py:17-27 (pairwise_NNs_inner) and :410-421 inside its own forward_loss / forward.

Like make_golden.py (whose reference import it uses) this runs ONLY where the reference is importable and copies none of it.  A model
is assembled as make_golden.gen_model assembles one, with loss-type 'matching-entropy' and loss-weights [1.0, 0.1], and once more with
the 'auto' weights of alad_model.py:271-273.  The reference runs in float64 (its code does not name a dtype), on the float32 inputs
widened, so the recorded values carry no float32 rounding of their own; its float32 run must pick the same neighbours (asserted).

    families   a  aligned: synth.global_embeddings(B, D, seed, 1.0), matched pairs, mutual cross-modal neighbours
               b  unaligned: image half of seed, caption half of an independent seed -- neighbours in all four quadrants, shared ones
               c  the self-neighbour case: img [[2, 0]], cap [[-2, 0]]: every off-diagonal product is -4 < -1, I = [0, 1]
    shapes     tests/helpers/entropy_numpy.py: SHAPES, families a and b at each
    condition  every row of every case: best minus second-best product >= 1e-4 in float64 (asserted); family b takes the first
               seed pair from (61, 161) upwards that meets it, and records it
    per case   seeds, input checksums, I (pairwise_NNs_inner called directly == the one forward_loss used), the entropy term, the
               matching term, the total, dict keys, logged keys, d entropy / d inputs and d total / d inputs from autograd; gradients
               as float32 (2^-24 relative, three orders below the GPU tolerance); of d entropy every 4th column where B * D > 4096, and
               d total (fixed and 'auto' weights) where B <= 33 only -- the file's size

    python tests/golden/make_golden_entropy.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'helpers'))

import numpy as np
import torch

import make_golden as MG                          # noqa: E402  (reference on the path, import_alad_model, t)
import entropy_numpy as E                         # noqa: E402
from aladin_amd import synth                      # noqa: E402

NAME = 'entropy'
LOSS_TYPE, WEIGHTS = 'matching-entropy', [1.0, 0.1]
SEED_A, SEED_B = 51, (61, 161)


def build_model(am, auto, dtype):
    tr = {'loss-type': LOSS_TYPE, 'loss-weights': 'auto' if auto else WEIGHTS, 'margin': 0.2, 'measure': 'dot', 'max-violation': True}
    m = am.ALADModel.__new__(am.ALADModel)
    torch.nn.Module.__init__(m)
    m.losses_types = LOSS_TYPE.split('-')
    if auto:                                       # alad_model.py:271-273, in the run's dtype
        m.losses_weights = {k: torch.nn.Parameter(-2.3 * torch.ones(1, dtype=dtype)) for k in m.losses_types}
    else:
        m.losses_weights = dict(zip(m.losses_types, WEIGHTS))
    m.auto_weight = auto
    m.config = {'training': tr}
    m.matching_criterion = MG.ref_loss.ContrastiveLoss(margin=tr['margin'], measure=tr['measure'], max_violation=tr['max-violation'])
    m.pdist = torch.nn.PairwiseDistance(2)         # alad_model.py:303
    m.logger = MG.ref_eval.LogCollector()
    m.Eiters = 0
    return m


def run(am, img, cap, auto, dtype):
    """the reference's forward on (img, cap) -> dict of what it returned and autograd gave"""
    B, D = img.shape
    a = MG.t(img).to(dtype).requires_grad_(True)
    b = MG.t(cap).to(dtype).requires_grad_(True)
    m = build_model(am, auto, dtype)
    used = []
    orig = am.pairwise_NNs_inner
    am.pairwise_NNs_inner = lambda x: used.append(orig(x)) or used[-1]          # the indices forward_loss itself used
    try:
        sets = (a, b, torch.zeros((1, B, D), dtype=dtype), torch.zeros((1, B, D), dtype=dtype), [1] * B, [1] * B, 0)
        m.forward_emb = lambda x, y: sets
        total, d = m.forward(None, None, epoch=0, distill_epoch=2)
    finally:
        am.pairwise_NNs_inner = orig
    direct = orig(torch.cat([a, b], 0).detach())
    assert len(used) == 1 and torch.equal(used[0], direct)
    ge = torch.autograd.grad(d['entropy'], (a, b), retain_graph=True)
    gt = torch.autograd.grad(total.sum(), (a, b))
    return dict(I=direct.numpy(), keys=list(d.keys()), vals=[float(v) for v in d.values()], total=float(total),
                logged=list(m.logger.meters.keys()), logged_n={k: int(v.count) for k, v in m.logger.meters.items() if k != 'Eit'},
                dimg_entropy=ge[0].numpy(), dcap_entropy=ge[1].numpy(), dimg_total=gt[0].numpy(), dcap_total=gt[1].numpy())


def main():
    am = MG.import_alad_model()
    cases = [('c', 1, 2, 0, 0)]
    for B, D in E.SHAPES:
        cases.append(('a', B, D, SEED_A, 0))
        s1, s2 = SEED_B
        while E.gaps(np.concatenate(E.case_inputs('b', B, D, s1, s2), 0)).min() < E.MIN_GAP:
            s1, s2 = s1 + 1, s2 + 1
        cases.append(('b', B, D, s1, s2))
    out = dict(n_cases=len(cases), loss_type=LOSS_TYPE, weights=np.array(WEIGHTS), min_gap=E.MIN_GAP,
               cases=np.array([[ord(f), B, D, s1, s2] for f, B, D, s1, s2 in cases], dtype=np.int64))
    for ci, (fam, B, D, s1, s2) in enumerate(cases):
        img, cap = E.case_inputs(fam, B, D, s1, s2)
        x = np.concatenate([img, cap], 0)
        gap = float(E.gaps(x).min())
        assert gap >= E.MIN_GAP, (fam, B, D, gap)
        r = run(am, img, cap, False, torch.float64)
        r32 = run(am, img, cap, False, torch.float32)
        ra = run(am, img, cap, True, torch.float64)
        assert np.array_equal(r['I'], r32['I']) and np.array_equal(r['I'], ra['I']) and np.array_equal(r['I'], E.neighbours(x))
        assert r['keys'] == ra['keys'] == ['matching', 'entropy'] and r['logged'] == ra['logged']
        N, I = 2 * B, r['I']
        quad = {(int(i >= B), int(j >= B)) for i, j in enumerate(I)}
        shared = N - len(set(I.tolist()))
        if fam == 'a' and D >= 64:
            assert (I == (np.arange(N) + B) % N).mean() > 0.9, 'aligned pairs are mostly mutual cross-modal neighbours'
        if fam == 'b' and B >= 32:
            assert len(quad) == 4 and shared >= 3, (quad, shared)
        if fam == 'c':
            assert I.tolist() == [0, 1] and not r['dimg_entropy'].any() and not r['dcap_entropy'].any()
        cols = E.grad_columns(B, D)
        p = 'c%d_' % ci
        out.update({p + 'img_checksum': synth.checksum(img), p + 'cap_checksum': synth.checksum(cap), p + 'gap': gap, p + 'I': I.astype(np.int64),
                    p + 'keys': np.array(r['keys']), p + 'vals': np.array(r['vals']), p + 'total': r['total'],
                    p + 'vals_f32run': np.array(r32['vals']), p + 'logged': np.array(r['logged']),
                    p + 'logged_n': np.array([r['logged_n'][k] for k in r['logged'] if k != 'Eit']),
                    p + 'auto_total': ra['total'], p + 'auto_vals': np.array(ra['vals'])})
        for k in ('dimg_entropy', 'dcap_entropy'):
            out[p + k] = r[k][:, cols].astype(np.float32)
        if B <= E.MODEL_MAX_B:                       # the model-level cases: gradients of the weighted total, fixed and 'auto' weights
            for k in ('dimg_total', 'dcap_total'):
                out[p + k] = r[k].astype(np.float32)
                out[p + 'auto_' + k] = ra[k].astype(np.float32)
        print('case %2d  %s  B %3d D %3d  seeds %3d %3d  min gap %.2e  quadrants %d  rows sharing a neighbour %3d  entropy %.6f (f32 run %.6f)  '
              'total %.6f  auto %.6f' % (ci, fam, B, D, s1, s2, gap, len(quad), shared, r['vals'][1], r32['vals'][1], r['total'], ra['total']))
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **out)
    print('%s %.1f KB' % (NAME, os.path.getsize(path) / 1024))
    rec = {'pairwise_NNs_inner': MG.signature_record(am.pairwise_NNs_inner), 'ALADModel.forward_loss': MG.signature_record(am.ALADModel.forward_loss)}
    with open(os.path.join(HERE, 'signatures_entropy.json'), 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print('signatures_entropy.json: %d callables' % len(rec))


if __name__ == '__main__':
    main()
