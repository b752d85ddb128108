"""Generate tests/golden/attdistill.npz and tests/golden/signatures_attdistill.json by running the REFERENCE (mesnico/ALADIN)
AttentionDistillationLoss, alad/loss.py:273-334.

Like make_golden_xent.py (whose conventions it follows) this runs ONLY where the reference is importable and copies none of it.
The reference runs in float64 on the float32 inputs widened.  Cases: tests/helpers/attdistill_numpy.py FIXTURE_CASES.

    'whole'      full-length images (the reference is finite there): its loss and both gradients on the batch
    'per_image'  ragged images, a teacher without mass on masked regions: on current PyTorch the reference's loss is NaN (0 * -inf in
                 kl_div) while its gradients are finite -- the gradients are recorded from the batch, the loss from the reference run
                 PER IMAGE on the set truncated to the image's valid length, averaged over the images (N = Bi * sum_j m_j makes the
                 batch loss that mean); the NaN of the batch run is asserted and recorded as a flag
    per case     the generator arguments (JSON), input checksums, loss, d im_set, d s_seq (float64)

    python tests/golden/make_golden_attdistill.py
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
import attdistill_numpy as A                      # noqa: E402
from aladin_amd import synth                      # noqa: E402

NAME = 'attdistill'


def run(im, s, im_len, s_len, teacher, want_grad=True):
    """the reference's criterion in float64 -> (loss, d_im, d_s)"""
    a = MG.t(im).to(torch.float64).requires_grad_(True)
    b = MG.t(s).to(torch.float64).requires_grad_(True)
    crit = MG.ref_loss.AttentionDistillationLoss()
    assert list(crit.state_dict()) == []
    loss = crit(a, b, list(im_len), list(s_len), MG.t(teacher).to(torch.float64))
    if not want_grad:
        return float(loss), None, None
    ga, gb = torch.autograd.grad(loss, (a, b))
    return float(loss), ga.numpy(), gb.numpy()


def main():
    rec = {'n_cases': np.int64(len(A.FIXTURE_CASES))}
    for ci, (name, how, kw) in enumerate(A.FIXTURE_CASES):
        x = A.make_inputs(**kw)
        im, s, im_len, s_len, teacher = x['im'], x['s'], x['im_len'], x['s_len'], x['teacher']
        loss, d_im, d_s = run(im, s, im_len, s_len, teacher)
        assert np.isfinite(d_im).all() and np.isfinite(d_s).all(), name
        batch_nan = not np.isfinite(loss)
        if how == 'per_image':
            assert batch_nan, (name, loss)
            n, _ = A.counts(im_len, s_len, im.shape[1] - 1, s.shape[1] - 1)
            assert (n >= 1).all()
            per = [run(im[i:i + 1, :n[i] + 1], s, [int(n[i]) + 1], s_len, teacher[i:i + 1, :, :, :n[i]], False)[0] for i in range(len(n))]
            assert np.isfinite(per).all()
            loss = float(np.mean(per))
        else:
            assert how == 'whole' and not batch_nan, (name, loss)
        pre = 'c%d_' % ci
        rec[pre + 'name'] = np.array(name)
        rec[pre + 'how'] = np.array(how)
        rec[pre + 'args'] = np.array(json.dumps(kw, sort_keys=True))
        rec[pre + 'batch_loss_nan'] = np.bool_(batch_nan)
        for key in ('im', 's', 'teacher'):
            rec[pre + key + '_checksum'] = np.float64(synth.checksum(x[key]))
        rec[pre + 'loss'] = np.float64(loss)
        rec[pre + 'd_im'] = d_im.astype(np.float64)
        rec[pre + 'd_s'] = d_s.astype(np.float64)
        print('%-32s %-9s loss %.12g  max|d_im| %.3g  max|d_s| %.3g' % (name, how, loss, np.abs(d_im).max(), np.abs(d_s).max()))
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **rec)
    print('%s: %d bytes' % (path, os.path.getsize(path)))
    sig = {'AttentionDistillationLoss.__init__': MG.signature_record(MG.ref_loss.AttentionDistillationLoss.__init__),
           'AttentionDistillationLoss.forward': MG.signature_record(MG.ref_loss.AttentionDistillationLoss.forward)}
    with open(os.path.join(HERE, 'signatures_%s.json' % NAME), 'w') as f:
        json.dump(sig, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
