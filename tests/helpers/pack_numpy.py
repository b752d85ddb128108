"""The packed operand format in float64, written from DESIGN.md section 3 and include/aladin_hip.h (struct aladin_align_geom, the
ALADIN_PRECISION_* and ALADIN_LAYOUT_* comments) -- not from the kernels.

    xm   (xm_rows, Dp)  image i at rows [i * mrows, (i + 1) * mrows): scored regions 0 .. R' - 1 are raw positions 1 .. R'; rows past
                        R' repeat region 0
    xe   (xe_rows, Dp)  image i at rows [i * rem, (i + 1) * rem): regions mrows .. mrows + rem - 1
    y    (y_rows, Dp)   caption j at rows [j * trows, (j + 1) * trows): scored words 0 .. T' - 1 are raw positions 1 .. T'
    rnorm               one value per row of [xm | xe | y]: 1 / max(|x|, 1e-12) of the raw vector, 0 for a zero row

A position counts when it is below clamp(len - 1 - tail, 0, R' or T'); every other row -- a masked position, a position past R' / T'
on the sum side, a sample that only pads a tile -- is zero.  Columns D .. Dp are zero.  What counts holds the unit vector.

expected(geom, im, s, il, sl) returns, for each of xm / xe / y, (unit, kind, inv) with
    unit  (rows, D) float64 unit vectors (0 on zero rows)
    kind  (rows,)   0 zero row, 1 a scored position, 2 a tile-filling copy of the sample's region 0
    inv   (rows,)   float64 1 / max(|x|, 1e-12), 0 on zero rows
"""
import numpy as np

ZERO, SCORED, COPY = 0, 1, 2


def scored_len(length, tail, cap):
    return min(max(int(length) - 1 - tail, 0), cap)


def max_side_rows(g):
    """[(operand, row, image, region, is_copy)] over xm then xe."""
    out = []
    for i in range(int(g.xm_rows) // g.mrows):
        for k in range(g.mrows):
            out.append(('xm', i * g.mrows + k, i, k if k < g.Rq else 0, k >= g.Rq))
    for row in range(int(g.xe_rows)):
        i, k = divmod(row, g.rem)
        out.append(('xe', row, i, g.mrows + k, False))
    return out


def sum_side_rows(g):
    """[(row, caption, word)] over y."""
    return [(j * g.trows + w, j, w) for j in range(int(g.y_rows) // g.trows) for w in range(g.trows)]


def _unit(x):
    x = x.astype(np.float64)
    inv = 1.0 / max(float(np.sqrt((x * x).sum())), 1e-12)
    return x * inv, inv


def expected(g, im, s, il, sl):
    D = g.D
    res = {}
    for name, rows in (('xm', int(g.xm_rows)), ('xe', int(g.xe_rows)), ('y', int(g.y_rows))):
        res[name] = [np.zeros((rows, D)), np.zeros(rows, np.int64), np.zeros(rows)]
    for op, row, i, rho, copy in max_side_rows(g):
        if i < g.Bi and rho < scored_len(il[i], g.x_tail, g.Rq):
            u, inv = _unit(im[i, rho + 1])
            res[op][0][row], res[op][1][row], res[op][2][row] = u, (COPY if copy else SCORED), inv
    for row, j, w in sum_side_rows(g):
        if j < g.Bc and w < scored_len(sl[j], g.y_tail, g.Tq):
            u, inv = _unit(s[j, w + 1])
            res['y'][0][row], res['y'][1][row], res['y'][2][row] = u, SCORED, inv
    return {k: tuple(v) for k, v in res.items()}


# ---- bounds of the issue "Packed operands: one row map, one normaliser, one pack kernel", per element against the float64 unit vector u
def fp16_bound(u, D):
    """half-ulp of a normal fp16 + a crude bound on the fp32 normalisation, relative; the fp16 subnormal floor, absolute"""
    return (2.0 ** -11 * (1 + 2.0 ** -10) + (D / 2 + 10) * 2.0 ** -24) * np.abs(u) + 2.0 ** -25


def split_bound(u, D):
    return (2.0 ** -22 * (1 + 2.0 ** -10) + (D / 2 + 10) * 2.0 ** -24) * np.abs(u) + 2.0 ** -39


def rnorm_rel_bound(D):
    return (D / 2 + 10) * 2.0 ** -24


SPLIT_SCALE = 2.0 ** 14
