"""ROUGE-L relevance computed on the GPU: the drop-in for alad/evaluate_utils/rouge.py, and the producer of the relevance matrix
that alad/evaluate_utils/compute_relevance.py writes with it.

    tokenize                                 the reference's caption.lower().split(" "), as token ids
    Rouge, Rouge.score                       <- alad/evaluate_utils/rouge.py:37-76
    my_lcs                                   <- alad/evaluate_utils/rouge.py:14-34
    relevance_matrix                         new: every caption of a split against every image, one device matrix
    write_relevance_file                     <- alad/evaluate_utils/compute_relevance.py (method 'rougeL'): the raw float32 file DCG maps

The reference fills the (captions x images) matrix with one Python LCS table per (query caption, reference caption) pair in a
multiprocessing pool; here ops.rouge_l_relevance (csrc/rouge.hip) scores every pair with a bit-parallel LCS and the reference's
double arithmetic, so the float32 words are the reference's.  Captions longer than 256 tokens are truncated to 256.

SPICE and METEOR relevances stay out of scope: they need the Java jar and coco_caption.
"""
import os

import numpy as np
import torch

from . import ops

CAPS_PER_IMG = 5


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('aladin_amd: ROUGE-L is computed by a HIP kernel on an MI355X only (no GPU visible, no CPU fallback exists)')
    return torch.device('cuda', torch.cuda.current_device())


def tokenize(captions, vocab=None):
    """-> (tokens int32 array, offsets int64 array of len(captions) + 1, vocab {token: id}).  A caption's tokens are
    caption.lower().split(" ") (rouge.py:59,63): the split is on the single space only, so doubled, leading or trailing spaces
    give empty-string tokens, the empty caption is the one token '', and tabs do not separate.  Ids are handed out in order of
    first appearance; `vocab` continues an earlier call's."""
    vocab = {} if vocab is None else vocab
    ids, offsets = [], [0]
    for c in captions:
        if not isinstance(c, str):
            raise TypeError('aladin_amd: a caption must be a str, got %r' % type(c))
        for t in c.lower().split(" "):
            ids.append(vocab.setdefault(t, len(vocab)))
        offsets.append(len(ids))
    return np.asarray(ids, dtype=np.int32), np.asarray(offsets, dtype=np.int64), vocab


class _Gallery:
    """The captions of a split on the device: every caption a gallery caption, image j owning captions caps_per_img * j ..."""

    def __init__(self, captions, caps_per_img):
        captions = list(captions)
        caps_per_img = int(caps_per_img)
        if caps_per_img < 1 or len(captions) == 0 or len(captions) % caps_per_img != 0:
            raise ValueError('aladin_amd: relevance_matrix needs a non-empty list of captions, %d per image (got %d captions)'
                             % (caps_per_img, len(captions)))
        self.tokens, self.offsets, _ = tokenize(captions)
        self.n_cap, self.n_img = len(captions), len(captions) // caps_per_img
        dev = _device()
        self.tok_d = torch.from_numpy(self.tokens).to(dev)
        self.off_d = torch.from_numpy(self.offsets).to(dev)
        self.grp_d = torch.arange(0, self.n_cap + 1, caps_per_img, dtype=torch.int64, device=dev)

    def rows(self, lo, hi):
        """Captions lo .. hi - 1 as queries against every image: a (hi - lo, n_img) float32 device tensor."""
        b, e = int(self.offsets[lo]), int(self.offsets[hi])
        return ops.rouge_l_relevance(self.tok_d[b:e], self.off_d[lo:hi + 1] - b, self.tok_d, self.off_d, self.grp_d)

    def listed(self, queries):
        idx = np.asarray(list(queries), dtype=np.int64).reshape(-1)
        if idx.size == 0 or idx.min() < 0 or idx.max() >= self.n_cap:
            raise ValueError('aladin_amd: relevance_matrix: queries must list captions 0 .. %d' % (self.n_cap - 1))
        lens = self.offsets[idx + 1] - self.offsets[idx]
        off = np.zeros(idx.size + 1, dtype=np.int64)
        off[1:] = np.cumsum(lens)
        tok = np.concatenate([self.tokens[self.offsets[i]:self.offsets[i + 1]] for i in idx])
        dev = self.tok_d.device
        return ops.rouge_l_relevance(torch.from_numpy(tok).to(dev), torch.from_numpy(off).to(dev), self.tok_d, self.off_d, self.grp_d)


def relevance_matrix(captions, caps_per_img=5, queries=None):
    """(n_cap, n_img) float32 device tensor, the layout of the reference's relevance file: row c = caption c as the query, column
    j = image j, whose references are captions caps_per_img * j .. caps_per_img * j + caps_per_img - 1.  A caption against its own
    image scores exactly 1.0.  queries: caption indices (any order) to compute only those rows, in that order."""
    g = _Gallery(captions, caps_per_img)
    return g.rows(0, g.n_cap) if queries is None else g.listed(queries)


def write_relevance_file(config, split, captions, method='rougeL', chunk=4096):
    """Write <data>/<name>/relevances/<name>-<split>-rougeL.npy, the raw float32 (captions x images) file that dcg.DCG maps (no
    .npy header: the reference writes a numpy.memmap), in chunks of `chunk` query rows so that the host never holds the matrix.
    -> the path."""
    if method != 'rougeL':
        raise ValueError('aladin_amd: only the rougeL relevance is computed here (got %r); SPICE and METEOR need the Java jar' % (method,))
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError('aladin_amd: write_relevance_file needs chunk >= 1')
    g = _Gallery(captions, CAPS_PER_IMG)
    name = config['dataset']['name']
    relevance_dir = os.path.join(config['dataset']['data'], name, 'relevances')
    os.makedirs(relevance_dir, exist_ok=True)
    path = os.path.join(relevance_dir, '{}-{}-{}.npy'.format(name, split, method))
    with open(path, 'wb') as f:
        for lo in range(0, g.n_cap, chunk):
            g.rows(lo, min(lo + chunk, g.n_cap)).cpu().numpy().tofile(f)
    return path


def _one_query(query_tokens, refs_tokens, lcs):
    """The kernel with one query and one image holding the references -> its float32 result as a Python float."""
    vocab = {}
    q = np.asarray([vocab.setdefault(t, len(vocab)) for t in query_tokens], dtype=np.int32)
    g, off = [], [0]
    for r in refs_tokens:
        g.extend(vocab.setdefault(t, len(vocab)) for t in r)
        off.append(len(g))
    dev = _device()
    out = ops.rouge_l_relevance(torch.from_numpy(q).to(dev), torch.tensor([0, len(q)], dtype=torch.int64, device=dev),
                                torch.from_numpy(np.asarray(g, dtype=np.int32)).to(dev), torch.tensor(off, dtype=torch.int64, device=dev),
                                torch.tensor([0, len(refs_tokens)], dtype=torch.int64, device=dev), lcs=lcs)
    return float(out.item())


def my_lcs(string, sub):
    """reference rouge.py:14-34: the length of the longest common subsequence of two token lists."""
    if len(string) == 0 or len(sub) == 0:
        return 0
    if max(len(string), len(sub)) > ops.ROUGE_MAX_LEN:
        raise ValueError('aladin_amd: my_lcs takes at most %d tokens a side' % ops.ROUGE_MAX_LEN)
    return int(_one_query(list(sub), [list(string)], True))


class Rouge:
    """reference rouge.py:37-76: ROUGE-L of one candidate sentence against an image's reference sentences."""

    def __init__(self):
        self.beta = 1.2              # the kernel's constant (csrc/rouge.hip); changing it here changes nothing

    def score(self, candidate, refs):
        """reference rouge.py:46-76: candidate = [sentence], refs = the image's sentences -> the F-measure as a Python float (the
        float32 value of the relevance file)."""
        assert (len(candidate) == 1)
        assert (len(refs) > 0)
        return _one_query(candidate[0].lower().split(" "), [r.lower().split(" ") for r in refs], False)
