"""Row scalings for the row-norm contract tests (tests/test_row_norms_cpu.py, tests/test_row_norms_gpu.py).

The reference L2-normalises every region and word (F.normalize, eps 1e-12, alad/loss.py:80-81) before it scores them, so the
scores do not depend on a row's length and the gradient of a row scales with 1 / |row|.  Two families of per-row factors:

  * powers of two, 2^k with k in [KMIN, KMAX] = [-30, 30].  Multiplying a float32 row by 2^k is exact, and every step of a
    normaliser -- the fma chain of the sum of squares, sqrtf, the divide, fmaxf against 1e-12 -- commutes with it exactly as
    long as nothing leaves the normal range.  So the unit vector of the scaled row has the SAME BITS, every score is bit-equal,
    and the gradient of the scaled row is exactly 2^-k times the gradient of the unscaled row.  Bounds, for the rows the tests
    use (standard normal at 40 <= D <= 1088, or three times that plus a shared direction at D <= 128; asserted on the inputs by
    assert_pow2_scaling_is_exact):
        - every non-zero component is at least 2^-30 in size, so its square times 2^-60 stays a normal float32;
        - a row's sum of squares stays within [2^-56, 2^71], its norm at or above 2^-28 = 3.7e-9 -- 3700 times the 1e-12 eps,
          and the comparison with the eps is an exact one, so no row changes sides;
        - the inverse norm stays within [2^-36, 2^28]; a gradient entry is a difference of O(1) sums of unit-vector components
          (resolution about 2^-24) times an inverse norm, so a non-zero entry is no smaller than about 2^-60, far above the
          float32 subnormals (2^-126): unscale_grad, a multiplication by 2^k, is exact and equality is meaningful.  The GPU tier
          asserts this on what it gets (assert_grad_unscaling_is_exact).
  * decades, 10^U(-3, 3): not powers of two, so the unit vectors are NOT bit-equal; for the comparison with the float64 oracle,
    where each gradient row is judged after multiplying it by its row's input norm (which removes the 1 / |row| factor).

On top of the random draw every case forces a fixed set of positions (forced_positions), chosen for the packed row map of
aladin_align_geometry (csrc/align_fwd.hip, csrc/pack_rows.hpp): rows whose inverse-norm slots are neighbours of rows with a very
different norm.  Positions are positions of the raw set: position p is scored row p - 1 (position 0 is dropped).
"""
import numpy as np

from aladin_amd import synth

KMIN, KMAX = -30, 30
K_SIDE = 17                      # the first side row: neither extreme, so that it differs from both of its neighbours' classes


def forced_positions(lens, tail, mrows=None, rem=0, half_tiles=False):
    """{(sample, position): exponent}, the adversarial positions of one side of an alignment problem.
    lens: the raw lengths; tail: trailing positions the side drops (images 0, captions 2), so that a sample's scored positions
    are 1 .. len - 1 - tail.  Rules, in this order; a position an earlier rule has set keeps its exponent:

      max side (mrows given: the rows an image has in the main operand; rem: its side rows):
        1. position 1 of every sample -> KMAX: region 1 is packed row 0, the row the tile-filling copies repeat;
        2. position min(mrows, longest scored length) of every sample -> KMIN: packed row mrows - 1, the last main row of the
           image (whose successor in the slot order is row 0 of the next image); in a class with tile-filling copies
           (fewer scored regions than main rows) the last scored region, whose successors are the copies of region 1;
        3. rem > 0: position mrows + 1 of every sample -> K_SIDE: side row 0, the first slot of the [xe] part;
        4. the last sample: its last scored position -> KMIN (its first is KMAX by rule 1).
      sum side (mrows None):
        1. half_tiles (captions packed into 8, 24 or 40 rows, two captions sharing a 16-word tile): the last scored position of
           sample 0 -> KMAX and position 1 of sample 1 -> KMIN: neighbours in one tile;
        2. the last sample: position 1 -> KMAX, its last scored position -> KMIN.
    Positions that do not exist (a set too short, a sample without scored positions) are left out."""
    lens = [int(v) for v in lens]
    last = [L - 1 - tail for L in lens]                     # last scored position per sample (< 1: none)
    out = {}

    def put(b, p, k):
        if 0 <= b < len(lens) and p >= 1 and (b, p) not in out:
            out[(b, p)] = k

    if mrows is not None:
        longest = max(last)
        for b in range(len(lens)):
            put(b, 1, KMAX)
        for b in range(len(lens)):
            put(b, min(mrows, longest), KMIN)
        if rem > 0:
            for b in range(len(lens)):
                put(b, mrows + 1, K_SIDE)
        put(len(lens) - 1, last[-1], KMIN)
    else:
        if half_tiles and len(lens) > 1:
            put(0, last[0], KMAX)
            put(1, 1, KMIN)
        b = len(lens) - 1
        put(b, 1, KMAX)
        put(b, last[b], KMIN)
    return out


def pow2_row_scales(shape_rows, seed, kmin=KMIN, kmax=KMAX, forced=None):
    """int64 exponents per (sample, position): uniform in [kmin, kmax] (aladin_amd.synth.integers), then the forced positions."""
    k = synth.integers(tuple(shape_rows), kmin, kmax, seed)
    for (b, p), e in (forced or {}).items():
        assert kmin <= e <= kmax and p < shape_rows[1], ((b, p), e, shape_rows)
        k[b, p] = e
    return k


def scale_rows(x, k):
    """x[b, p, :] * 2^k[b, p], exact."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.shape[:-1] == k.shape
    return np.ldexp(x, np.asarray(k)[..., None].astype(np.int32)).astype(np.float32)


def unscale_grad(g, k):
    """g[b, p, :] * 2^k[b, p]: maps the gradient of a scaled row back to the gradient of the unscaled row, exactly."""
    g = np.asarray(g)
    assert g.shape[:-1] == k.shape
    return np.ldexp(g, np.asarray(k)[..., None].astype(np.int32)).astype(g.dtype)


def assert_pow2_scaling_is_exact(x, k):
    """The bounds of the module docstring, on the inputs of a case: x (float32 rows) and the exponents k."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and np.abs(k).max() <= max(-KMIN, KMAX)
    nz = np.abs(x[x != 0])
    assert nz.size and nz.min() >= 2.0 ** -30, nz.min()
    xs = scale_rows(x, k)
    assert np.array_equal(np.ldexp(xs, -np.asarray(k)[..., None].astype(np.int32)), x)        # nothing was rounded or flushed
    ss = (xs.astype(np.float64) ** 2).sum(-1)
    live = ss > 0
    assert ss[live].min() >= 2.0 ** -56 and ss[live].max() <= 2.0 ** 71, (ss[live].min(), ss[live].max())
    assert np.sqrt(ss[live].min()) >= 2.0 ** -28


def assert_grad_unscaling_is_exact(g_scaled):
    """A scaled row's gradient must not have met the subnormals, or 2^k times it is not the unscaled gradient's bits."""
    g = np.abs(np.asarray(g_scaled, np.float64))
    assert np.isfinite(g).all()
    nz = g[g != 0]
    assert nz.size == 0 or nz.min() >= 2.0 ** -100, nz.min()


def decade_row_scales(shape_rows, seed):
    """float64 factors 10^U(-3, 3) per (sample, position); none is a power of two."""
    f = 10.0 ** (6.0 * synth.uniform(tuple(shape_rows), seed) - 3.0)
    m, _ = np.frexp(f)
    assert (m != 0.5).all()
    return f


def scale_rows_by(x, f):
    """x[b, p, :] * f[b, p] rounded to float32: the inputs BOTH the kernels and the oracle are given."""
    x = np.asarray(x)
    assert x.shape[:-1] == f.shape
    return (x.astype(np.float64) * f[..., None]).astype(np.float32)


def row_norms(x):
    """float64 norms (B, N, 1) of the rows of x."""
    return np.sqrt((np.asarray(x, np.float64) ** 2).sum(-1, keepdims=True))


# ------------------------------------------------------------------------------------------------
# the cases both tiers use: shapes (Bi, Bc, R, T, D), each there for its packed row map
# ------------------------------------------------------------------------------------------------
TILE_SHAPES = [
    (5, 7, 34, 20, 64),        # 32 rows + 1 side row, 24-word half class
    (6, 5, 51, 38, 128),       # 48 rows + 2 side rows, 40-word half class
    (5, 6, 42, 11, 72),        # 48-row class with tile-filling copies (41 regions), 8-word half class, D no multiple of 64
    (4, 4, 57, 90, 64),        # 48 rows + 8 side rows, six word tiles
    (4, 5, 66, 36, 64),        # two region tiles + one side row (65 regions), 40-word half class
    (3, 4, 71, 71, 64),        # 96 rows, no side rows: the 32x32 body
    (9, 4, 17, 9, 40),         # one padded region tile, D % 8 != 0: the scalar packer
]
FORWARD_ONLY_SHAPE = (3, 3, 34, 20, 1088)        # the streamed packer; the backward stops at D = 1024
LONG_SHAPES = [(5, 6, 98, 50, 64), (6, 5, 34, 100, 64)]      # the two smallest of tests/test_long_sets_gpu.py: long images, long captions
# main rows per image, side rows per image, rows per caption -- the class comment of aladin_align_geometry (csrc/align_fwd.hip)
# and, for the long layout, csrc/align_long.hip (32-row / 16-word multiples, no side rows)
EXPECTED_ROW_MAP = {
    (5, 7, 34, 20, 64): (32, 1, 24), (6, 5, 51, 38, 128): (48, 2, 40), (5, 6, 42, 11, 72): (48, 0, 8), (4, 4, 57, 90, 64): (48, 8, 96),
    (4, 5, 66, 36, 64): (64, 1, 40), (3, 4, 71, 71, 64): (96, 0, 96), (9, 4, 17, 9, 40): (32, 0, 8), (3, 3, 34, 20, 1088): (32, 1, 24),
    (5, 6, 98, 50, 64): (128, 0, 48), (6, 5, 34, 100, 64): (64, 0, 112),
    (10, 10, 51, 38, 128): (48, 2, 40), (12, 12, 34, 50, 64): (32, 1, 48), (128, 128, 51, 38, 128): (48, 2, 40), (128, 128, 34, 50, 64): (32, 1, 48),
    (8, 8, 34, 50, 64): (32, 1, 48), (33, 33, 34, 50, 64): (32, 1, 48),
}


def ragged_lengths(B, N, tail, seed, lo, tile):
    """U{lo..N} lengths with sample 0 at full length, sample 1 one short of it and (where it exists) sample 2 filling exactly
    `tile` scored positions."""
    lens = [int(v) for v in synth.integers((B,), min(lo, N), N, seed)]
    lens[0] = N
    if B > 1:
        lens[1] = N - 1
    if B > 2 and tile + 1 + tail <= N:
        lens[2] = tile + 1 + tail
    return lens


_CASES = {}


def alignment_case(shape, structured=False):
    """The case of a shape (cached): the base inputs (im, s), their power-of-two (im2, s2; exponents kx, ky) and decade (im10, s10;
    factors fx, fy) scalings, the lengths, an upstream gradient w and the row map.  The arrays are shared between tests: read-only.
    structured: caption i correlates with image i (synth.structured_alignment_batch's construction, noise 3), for the hinge
    losses."""
    import types
    from aladin_amd import ops
    key = (tuple(shape), structured)
    if key in _CASES:
        return _CASES[key]
    Bi, Bc, R, T, D = shape
    seed = 9000 + 131 * Bi + 17 * R + T + D
    g = ops.align_geometry(Bi, Bc, R, T, D, layout='auto')
    c = types.SimpleNamespace()
    c.shape, c.mrows, c.rem, c.trows, c.Rq, c.Tq = tuple(shape), int(g.mrows), int(g.rem), int(g.trows), int(g.Rq), int(g.Tq)
    c.half_tiles = c.trows % 16 == 8
    im, s = synth.normal((Bi, R, D), seed), synth.normal((Bc, T, D), seed + 4444)
    if structured:
        assert Bi == Bc
        base = synth.normal((Bi, 1, D), seed + 99)
        im, s = (im * 3.0 + base).astype(np.float32), (s * 3.0 + base).astype(np.float32)
    c.im, c.s = im, s
    c.il = ragged_lengths(Bi, R, 0, seed + 17, 10, c.mrows)
    c.sl = ragged_lengths(Bc, T, 2, seed + 29, 6, 16)
    c.forced_x = forced_positions(c.il, 0, c.mrows, c.rem)
    c.forced_y = forced_positions(c.sl, 2, None, 0, c.half_tiles)
    c.kx = pow2_row_scales((Bi, R), seed + 1, forced=c.forced_x)
    c.ky = pow2_row_scales((Bc, T), seed + 2, forced=c.forced_y)
    assert_pow2_scaling_is_exact(im, c.kx)
    assert_pow2_scaling_is_exact(s, c.ky)
    c.im2, c.s2 = scale_rows(im, c.kx), scale_rows(s, c.ky)
    c.fx, c.fy = decade_row_scales((Bi, R), seed + 3), decade_row_scales((Bc, T), seed + 4)
    c.im10, c.s10 = scale_rows_by(im, c.fx), scale_rows_by(s, c.fy)
    c.w = (synth.normal((Bi, Bc), seed + 7) * (synth.uniform((Bi, Bc), seed + 8) < 0.5)).astype(np.float32)
    for a in (c.im, c.s, c.kx, c.ky, c.im2, c.s2, c.fx, c.fy, c.im10, c.s10, c.w):
        a.setflags(write=False)
    _CASES[key] = c
    return c
