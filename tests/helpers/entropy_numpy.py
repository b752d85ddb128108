"""A numpy restatement, in float64, of the 'entropy' loss term that aladin_nn_entropy_fwd / _bwd compute (include/aladin_hip.h):
reference alad/alad_model.py:17-27 (pairwise_NNs_inner) and :410-421, with the one rule the reference leaves open stated -- ties of
the row maximum go to the lowest index (numpy's argmax).  Also the inputs of tests/golden/entropy.npz, rebuilt from their seeds.
tests/test_entropy_cpu.py pins it to the reference's recorded values; the GPU tests use it where the fixture keeps a part only."""
import numpy as np

EPS = 1e-6                           # nn.PairwiseDistance's eps, added to the difference inside the norm
MIN_GAP = 1e-4                       # least gap between a row's best and second-best product in every fixture case

# (B, D) of the fixture's families (a) and (b)
SHAPES = [(1, 8), (3, 8), (32, 64), (33, 70), (64, 64), (96, 768), (130, 100)]
GRAD_COLUMN_STEP = 4                 # cases with B * D > GRAD_FULL_MAX record every 4th gradient column (the 1 MiB limit on a file)
GRAD_FULL_MAX = 4096
MODEL_MAX_B = 33                     # cases up to this B also record the gradients of the model's weighted total


def case_inputs(family, B, D, seed, seed2=0):
    """(img, cap) float32 of a fixture case.  'a' aligned: matched pairs of one synth.global_embeddings draw;  'b' unaligned: the
    image half of the draw `seed`, the caption half of the independent draw `seed2`;  'c': the self-neighbour case, fixed values."""
    from aladin_amd import synth
    if family == 'c':
        return np.array([[2.0, 0.0]], np.float32), np.array([[-2.0, 0.0]], np.float32)
    img, cap = synth.global_embeddings(B, D, seed, 1.0)
    if family == 'b':
        cap = synth.global_embeddings(B, D, seed2, 1.0)[1]
    return img, cap


def grad_columns(B, D):
    """the gradient columns a fixture case records"""
    return slice(None, None, GRAD_COLUMN_STEP if B * D > GRAD_FULL_MAX else 1)


def products(x):
    """x @ x.T in float64 with the reference's diagonal: -1, not -inf."""
    x = np.asarray(x, dtype=np.float64)
    dots = x @ x.T
    np.fill_diagonal(dots, -1.0)
    return dots


def neighbours(x):
    """pairwise_NNs_inner: the other row of largest inner product, lowest index on ties; a row whose other products are all below
    -1 is its own neighbour."""
    return np.argmax(products(x), axis=1)


def gaps(x):
    """per row: best minus second-best product (inf for a single candidate); what decides whether arg-max parity can be asked"""
    dots = np.sort(products(x), axis=1)
    return dots[:, -1] - dots[:, -2] if dots.shape[1] > 1 else np.full(len(dots), np.inf)


def entropy_loss(img, cap, g=1.0):
    """-> (loss, nn, dist, d_img, d_cap): loss = -mean_i log(N * dist_i), dist_i = ||x_i - x_nn(i) + eps||, and g * dloss/d(img, cap)
    with no gradient through the neighbour choice: c_i * u_i added to row i and subtracted from row nn(i), c_i = -g / (N dist_i^2)."""
    img, cap = np.asarray(img, dtype=np.float64), np.asarray(cap, dtype=np.float64)
    x = np.concatenate([img, cap], 0)
    N = len(x)
    nn = neighbours(x)
    u = x - x[nn] + EPS
    dist = np.sqrt((u * u).sum(1))
    loss = -np.mean(np.log(N * dist))
    cu = (-g / (N * dist * dist))[:, None] * u
    grad = cu.copy()
    np.subtract.at(grad, nn, cu)                  # a self-neighbour row: cu - cu = exactly 0
    return loss, nn, dist, grad[:len(img)], grad[len(img):]
