"""Generate tests/golden/xent.npz and tests/golden/signatures_xent.json by running the REFERENCE (mesnico/ALADIN)
CrossEntropyCriterion, alad/loss.py:190-201.

Like make_golden_entropy.py (whose conventions it follows) this runs ONLY where the reference is importable and copies none of it.
The reference runs in float64 (its code does not name a dtype) on the float32 inputs widened, its `temperature` set to the case's
value, so the recorded values carry no float32 rounding of their own; its float32 run is recorded beside it for orientation.

    shapes        tests/helpers/xent_numpy.py: SHAPES, each at the TEMPERATURES t in {0, 1.5, ln 100 as a float32}
    families      matched      synth.global_embeddings(B, D, seed, MATCHED_NOISE): matched pairs, a sharp diagonal
                  independent  image half of one draw, caption half of an independent one
    condition     every case with B > 1: the largest off-diagonal softmax mass of any row or column >= MIN_TOP_MASS (asserted) --
                  the reference's softmax - 1 is rounded at 1e-16 absolute, see xent_numpy.MIN_TOP_MASS
    per case      seeds, input checksums, loss, d loss / d im, d s, d temperature from autograd; gradients as float32 (2^-24
                  relative), every 4th column of d im / d s where B * D > 4096 (make_golden_entropy.py's rule: the file's size)
    model cases   B <= MODEL_MAX_B: loss-type 'matching-crossentropy' with weights [1.0, 0.5] and with 'auto'.  The reference's model
                  has no branch for the token, so the expected total is assembled HERE by its weighting rule (alad_model.py:445-453:
                  sum_k w_k L_k, or 0.5 sum_k (L_k e^-w_k + w_k) with w_k = -2.3) from the reference's own ContrastiveLoss(margin 0.2,
                  'dot', max_violation) and CrossEntropyCriterion values, in the dict order matching, crossentropy; recorded with its
                  gradients in im, s and the temperature.

    python tests/golden/make_golden_xent.py
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

import make_golden as MG                          # noqa: E402  (reference on the path: ref_loss, t, signature_record)
import xent_numpy as X                            # noqa: E402
from aladin_amd import synth                      # noqa: E402

NAME = 'xent'
MARGIN = 0.2


def run(img, cap, t, dtype):
    """the reference's criterion on (img, cap) at temperature t -> (loss, d_im, d_s, d_t)"""
    a = MG.t(img).to(dtype).requires_grad_(True)
    b = MG.t(cap).to(dtype).requires_grad_(True)
    crit = MG.ref_loss.CrossEntropyCriterion().to(dtype)
    with torch.no_grad():
        crit.temperature.fill_(t)
    assert list(crit.state_dict()) == ['temperature'] and tuple(crit.temperature.shape) == (1,)
    loss = crit(a, b)
    ga, gb, gt = torch.autograd.grad(loss, (a, b, crit.temperature))
    return float(loss), ga.numpy(), gb.numpy(), float(gt)


def run_model(img, cap, t, auto):
    """the weighted total of 'matching-crossentropy' by the reference's rule, float64 -> dict"""
    dtype = torch.float64
    a = MG.t(img).to(dtype).requires_grad_(True)
    b = MG.t(cap).to(dtype).requires_grad_(True)
    mc = MG.ref_loss.ContrastiveLoss(margin=MARGIN, measure='dot', max_violation=True)
    xc = MG.ref_loss.CrossEntropyCriterion().to(dtype)
    with torch.no_grad():
        xc.temperature.fill_(t)
    d = {'matching': mc(a, b), 'crossentropy': xc(a, b)}
    keys = X.MODEL_LOSS_TYPE.split('-')
    assert list(d) == keys
    if auto:                                       # alad_model.py:271-273 and :445-449, in the run's dtype
        w = {k: torch.nn.Parameter(-2.3 * torch.ones(1, dtype=dtype)) for k in keys}
        total = 0
        for k in d:
            total = total + d[k] * torch.exp(-w[k]) + w[k]
        total = total * 0.5
    else:                                          # :450-453
        w = dict(zip(keys, X.MODEL_WEIGHTS))
        total = 0
        for k in d:
            total = total + d[k] * w[k]
    ga, gb, gt = torch.autograd.grad(total.sum(), (a, b, xc.temperature))
    return dict(vals=[float(v) for v in d.values()], total=float(total), dimg=ga.numpy(), dcap=gb.numpy(), dt=float(gt))


def main():
    cases = X.fixture_cases()
    out = dict(n_cases=len(cases), min_top_mass=X.MIN_TOP_MASS, matched_noise=X.MATCHED_NOISE, model_loss_type=X.MODEL_LOSS_TYPE,
               model_weights=np.array(X.MODEL_WEIGHTS), model_margin=MARGIN,
               cases=np.array([[X.FIXTURE_FAMILIES.index(f), B, D, s1, s2] for f, B, D, t, s1, s2 in cases], dtype=np.int64),
               temperatures=np.array([t for _, _, _, t, _, _ in cases], dtype=np.float64))
    for ci, (fam, B, D, t, s1, s2) in enumerate(cases):
        assert float(np.float32(t)) == t, 'the temperature is a float32 value'
        img, cap = X.case_inputs(fam, B, D, s1, s2)
        S = img.astype(np.float64) @ cap.astype(np.float64).T
        top_mass = float(X.offdiag_mass(S, t).max())
        assert B == 1 or top_mass >= X.MIN_TOP_MASS, (fam, B, D, t, top_mass)
        loss, d_im, d_s, d_t = run(img, cap, t, torch.float64)
        r32 = run(img, cap, t, torch.float32)
        mine = X.criterion_f64(img, cap, t)
        assert abs(mine[0] - loss) <= 1e-12 * max(1.0, abs(loss)) and abs(mine[3] - d_t) <= 1e-12 * max(1.0, abs(d_t))
        cols = X.grad_columns(B, D)
        p = 'c%d_' % ci
        out.update({p + 'img_checksum': synth.checksum(img), p + 'cap_checksum': synth.checksum(cap), p + 'top_mass': top_mass,
                    p + 'loss': loss, p + 'dt': d_t, p + 'dimg': d_im[:, cols].astype(np.float32), p + 'dcap': d_s[:, cols].astype(np.float32),
                    p + 'f32run': np.array([r32[0], r32[3]])})
        line = 'case %2d  %-11s B %3d D %3d t %.4f  top mass %.2e  loss %.9g (f32 run %.9g)  dt %.9g (f32 run %.9g)' % (
            ci, fam, B, D, t, top_mass, loss, r32[0], d_t, r32[3])
        if B <= X.MODEL_MAX_B:
            for auto in (False, True):
                r = run_model(img, cap, t, auto)
                q = p + ('auto_' if auto else '')
                out.update({q + 'vals': np.array(r['vals']), q + 'total': r['total'], q + 'dt_total': r['dt'],
                            q + 'dimg_total': r['dimg'].astype(np.float32), q + 'dcap_total': r['dcap'].astype(np.float32)})
                line += '  %s total %.6f' % ('auto' if auto else 'fixed', r['total'])
        print(line)
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **out)
    print('%s %.1f KB' % (NAME, os.path.getsize(path) / 1024))
    crit = MG.ref_loss.CrossEntropyCriterion
    rec = {'CrossEntropyCriterion.__init__': MG.signature_record(crit.__init__), 'CrossEntropyCriterion.forward': MG.signature_record(crit.forward)}
    with open(os.path.join(HERE, 'signatures_xent.json'), 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print('signatures_xent.json: %d callables' % len(rec))


if __name__ == '__main__':
    main()
