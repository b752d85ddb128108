"""Generate tests/golden/align_long_b4.npz by running the REFERENCE (mesnico/ALADIN) on a long-set problem.

Like make_golden.py this runs ONLY where the reference is importable (read-only); the GPU tier holds the HIP path to the file
it writes.  The inputs are regenerated from aladin_amd.synth (generator arguments and checksums are stored), the outputs are the
reference's: 'MrSw' scores, the max_violation=True loss and the gradients of both sets -- past the 96 scored positions per set of
the tile classes on both sides (129 regions, 117 words).

    python tests/golden/make_golden_long.py
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ.get('ALADIN_REFERENCE', '/root/reference'))
warnings.filterwarnings('ignore')

import numpy as np
import torch

from aladin_amd import synth

import alad.loss as ref_loss                      # noqa: E402

NAME = 'align_long_b4'
KIND, B, R, T, D, SEED, MARGIN = 'random', 4, 130, 120, 64, 41, 0.2


def main():
    im, s, im_len, s_len = synth.alignment_batch(B, R, T, D, SEED, ragged=True)
    out = dict(kind=KIND, B=B, Bc=B, R=R, T=T, D=D, seed=SEED, ragged=True, margin=MARGIN,
               im_len=np.array(im_len), s_len=np.array(s_len),
               im_checksum=synth.checksum(im), s_checksum=synth.checksum(s))
    crit = ref_loss.AlignmentContrastiveLoss(margin=MARGIN, measure='dot', max_violation=True, aggregation='MrSw')
    a = torch.from_numpy(im).requires_grad_(True)
    b = torch.from_numpy(s).requires_grad_(True)
    loss, S = crit(a, b, im_len, s_len, return_similarity_mat=True)
    loss.backward()
    out['S_MrSw'] = S.detach().numpy()
    out['loss_mv'] = loss.item()
    out['dim_mv'] = a.grad.numpy()
    out['ds_mv'] = b.grad.numpy()
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **out)
    print('%-28s %8.1f KB  im_len %s  s_len %s' % (NAME, os.path.getsize(path) / 1024, im_len, s_len))


if __name__ == '__main__':
    main()
