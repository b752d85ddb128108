"""Generate tests/golden/semantic.npz and tests/golden/signatures_semantic.json by running the REFERENCE (mesnico/ALADIN)
SemanticContrastiveLoss, alad/loss.py:203-270.

Like make_golden_xent.py (whose conventions it follows) this runs ONLY where the reference is importable and copies none of it.
The reference runs in float64 on the float32 inputs widened.  Its 2B calls of torch.randint(n, (1,)) are answered, for the
duration of the call, by recorded draws: the k-th call returns draws[k] % n (rows first, then columns -- the order of its two
loops), and exactly 2B draws must have been consumed.

    matrix level  compute_semantic_contrastive_loss(scores, relevances) at B in semantic_numpy.SIZES, every family of
                  semantic_numpy.FAMILIES, sum and max_violation mode, margin 0.2, threshold 0.4; scores on the 2^-16 grid
    class level   forward(im, s, relevances) for semantic_numpy.CLASS_CASES (measure, B, D), embeddings on the 2^-6 grid
    seeds         per case the first seed at which the INPUT CONDITION of semantic_numpy holds in both modes (asserted again here)
    per case      seed, input checksums, draws, the candidate counts the reference asked randint for, loss, dS = d loss / d scores
                  from autograd as int16 (asserted integer valued), the chosen positives (the restatement's, each checked against
                  the reference's randint call: same candidate count), min |x| and min top-two gap; class level: d im, d s (float32)

    python tests/golden/make_golden_semantic.py
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
import semantic_numpy as X                        # noqa: E402

NAME = 'semantic'


class RecordedDraws:
    """stands in for torch.randint while the reference runs: the k-th call (high, (1,)) -> draws[k] % high"""

    def __init__(self, draws):
        self.draws, self.k, self.asked = [int(d) for d in draws], 0, []

    def __call__(self, high, size, *a, **kw):
        assert tuple(size) == (1,) and not a and not kw and high > 0, (high, size, a, kw)
        r = self.draws[self.k] % int(high)
        self.k += 1
        self.asked.append(int(high))
        return torch.tensor([r], dtype=torch.int64)


def run_reference(call, draws, B):
    """call() with torch.randint answered from `draws` -> (call's result, the candidate counts asked for)"""
    fake, real = RecordedDraws(draws), torch.randint
    torch.randint = fake
    try:
        out = call()
    finally:
        torch.randint = real
    assert fake.k == 2 * B == len(draws), (fake.k, B)
    return out, np.array(fake.asked, np.int32)


def record(out, p, S64, rel, draws, loss, dS, asked, max_violation):
    """checks a reference run against the restatement's positives and files it under prefix p"""
    B = S64.shape[0]
    pos = X.positives(rel, X.THRESHOLD, draws)
    with np.errstate(invalid='ignore'):
        cand = rel > X.THRESHOLD
    assert np.array_equal(asked, np.concatenate([cand.sum(1), cand.sum(0)])), 'the reference counted other candidates'
    assert np.array_equal(dS, np.round(dS)) and np.abs(dS).max(initial=0) < 32768
    min_x, gap, ok = X.condition_figures(S64, rel, X.MARGIN, X.THRESHOLD, draws, max_violation)
    assert ok, (p, min_x, gap)
    mine = X.semantic_f64(S64, rel, X.MARGIN, X.THRESHOLD, draws, max_violation)
    assert abs(mine[0] - loss) <= 1e-11 * max(1.0, abs(loss)) and np.array_equal(mine[1], dS), p
    out.update({p + 'loss': loss, p + 'dS': dS.astype(np.int16), p + 'pos': pos.astype(np.int32), p + 'asked': asked,
                p + 'min_x': min_x, p + 'min_gap': gap})
    return min_x, gap


def main():
    out = dict(margin=X.MARGIN, threshold=X.THRESHOLD, cond_eps=X.COND_EPS,
               matrix_cases=np.array([[B, X.FAMILIES.index(f)] for B, f in X.matrix_cases()], dtype=np.int64),
               class_cases=np.array([[['dot', 'cosine', 'order'].index(m), B, D] for m, B, D in X.CLASS_CASES], dtype=np.int64))
    seeds = []
    for ci, (B, fam) in enumerate(X.matrix_cases()):
        seed = X.first_good_seed(lambda s: X.matrix_inputs(B, fam, s))
        seeds.append(seed)
        S, rel, draws = X.matrix_inputs(B, fam, seed)
        out.update({'m%d_S_checksum' % ci: X.checksum(S), 'm%d_rel_checksum' % ci: X.checksum(rel), 'm%d_draws' % ci: draws})
        for mv in X.MODES:
            crit = MG.ref_loss.SemanticContrastiveLoss(margin=X.MARGIN, threshold=X.THRESHOLD, measure='dot', max_violation=mv)
            sc = MG.t(S).to(torch.float64).requires_grad_(True)
            loss, asked = run_reference(lambda: crit.compute_semantic_contrastive_loss(sc, MG.t(rel)), draws, B)
            (g,) = torch.autograd.grad(loss, sc) if loss.requires_grad else (torch.zeros_like(sc),)
            min_x, gap = record(out, 'm%d_%s_' % (ci, 'max' if mv else 'sum'), S.astype(np.float64), rel, draws, float(loss), g.numpy(), asked, mv)
            print('matrix %2d  B %3d %-6s %s seed %d  loss %.9g  min|x| %.3g  min gap %.3g' % (ci, B, fam, 'max' if mv else 'sum', seed, float(loss),
                                                                                         min_x, gap))
    out['matrix_seeds'] = np.array(seeds, dtype=np.int64)
    seeds = []
    for ci, (measure, B, D) in enumerate(X.CLASS_CASES):
        def build(s):
            im, cap, rel, draws = X.class_inputs(measure, B, D, s)
            return X.class_scores(measure, im, cap), rel, draws
        seed = X.first_good_seed(build)
        seeds.append(seed)
        im, cap, rel, draws = X.class_inputs(measure, B, D, seed)
        out.update({'c%d_im_checksum' % ci: X.checksum(im), 'c%d_s_checksum' % ci: X.checksum(cap), 'c%d_rel_checksum' % ci: X.checksum(rel),
                    'c%d_draws' % ci: draws})
        for mv in X.MODES:
            crit = MG.ref_loss.SemanticContrastiveLoss(margin=X.MARGIN, threshold=X.THRESHOLD, measure=measure, max_violation=mv)
            a = MG.t(im).to(torch.float64).requires_grad_(True)
            b = MG.t(cap).to(torch.float64).requires_grad_(True)
            (loss, sc), asked = run_reference(lambda: crit(a, b, MG.t(rel), return_similarity_mat=True), draws, B)
            g, ga, gb = torch.autograd.grad(loss, (sc, a, b), allow_unused=True) if loss.requires_grad else (torch.zeros_like(sc), None, None)
            ga = torch.zeros_like(a) if ga is None else ga
            gb = torch.zeros_like(b) if gb is None else gb
            S64 = sc.detach().numpy()
            assert np.abs(S64 - X.class_scores(measure, im, cap)).max() <= 1e-12
            p = 'c%d_%s_' % (ci, 'max' if mv else 'sum')
            min_x, gap = record(out, p, S64, rel, draws, float(loss), g.numpy(), asked, mv)
            out.update({p + 'dim': ga.numpy().astype(np.float32), p + 'ds': gb.numpy().astype(np.float32)})
            print('class  %2d  %-6s (%2d, %2d) %s seed %d  loss %.9g  min|x| %.3g  min gap %.3g' % (ci, measure, B, D, 'max' if mv else 'sum', seed,
                                                                                              float(loss), min_x, gap))
    out['class_seeds'] = np.array(seeds, dtype=np.int64)
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **out)
    print('%s %.1f KB' % (NAME, os.path.getsize(path) / 1024))
    crit = MG.ref_loss.SemanticContrastiveLoss
    rec = {'SemanticContrastiveLoss.__init__': MG.signature_record(crit.__init__),
           'SemanticContrastiveLoss.forward': MG.signature_record(crit.forward),
           'SemanticContrastiveLoss.compute_semantic_contrastive_loss': MG.signature_record(crit.compute_semantic_contrastive_loss)}
    with open(os.path.join(HERE, 'signatures_semantic.json'), 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print('signatures_semantic.json: %d callables' % len(rec))


if __name__ == '__main__':
    main()
