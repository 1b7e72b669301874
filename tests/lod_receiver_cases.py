"""The numpy yardstick of the receivers on the LOD space (slod_lod_receivers_create, slod_lod_observe_*): the row of a term
from a lod_cases._slab_geometry, written as the loop of the reconstruction; the bilinear terms of a point; the value
y = O u in np.longdouble with its S_abs and term count for lod_cases._slab_bar.  Nothing here calls the library."""
import numpy as np


def term_row(geom, node):
    """(patch ids [m], ix [m], iy [m]) of the patches whose closed extent holds the fine node, in the order of the
    reconstruction: the centre cells cy, then cx, over the clipped range, a patch whose extent does not hold the node
    skipped."""
    n, l, N = geom.n, geom.l, geom.N
    X, Y = node % geom.NEp, node // geom.NEp
    cxl, cxh = max((X + n - 1) // n - 1 - l, 0), min(X // n + l, N - 1)
    cyl, cyh = max((Y + n - 1) // n - 1 - l, 0), min(Y // n + l, N - 1)
    ps, ixs, iys = [], [], []
    for cy in range(cyl, cyh + 1):
        for cx in range(cxl, cxh + 1):
            p = geom.pid[(cx, cy)]
            x0, y0, mx, my = (int(v) for v in geom.ext[p])
            ix, iy = X - x0 * n, Y - y0 * n
            if ix < 0 or ix > mx * n or iy < 0 or iy > my * n:
                continue
            ps.append(p), ixs.append(ix), iys.append(iy)
    return np.array(ps, dtype=np.int64), np.array(ixs, dtype=np.int64), np.array(iys, dtype=np.int64)


def term_columns(geom, node):
    """The columns p s + d of the row of a term at `node`, in row order."""
    ps, _, _ = term_row(geom, node)
    return (ps[:, None] * geom.s + np.arange(geom.s)[None, :]).ravel()


def term_offsets(geom, node, comp, stride):
    """The slab offsets of the words phi_{p,d}(node, comp) of the row, in row order (member 0, uniform stride)."""
    ps, ix, iy = term_row(geom, node)
    s, n = geom.s, geom.n
    pnx = geom.ext[ps, 2] * n + 1
    pnf = geom.n_fine[ps]
    d = np.arange(s)[None, :]
    return (ps[:, None] * stride + d * pnf[:, None] + (s * (ix + iy * pnx))[:, None] + comp).ravel()


def term_values(geom, vecs, node, comp):
    """phi_{p,d}(node, comp) of the row from vecs[p][d, iy, ix, c] (lod_cases._random_slab), in row order."""
    ps, ix, iy = term_row(geom, node)
    return np.array([vecs[p][d, y, x, comp] for p, x, y in zip(ps, ix, iy) for d in range(geom.s)])


def receiver_rows(geom, vecs, receivers):
    """CSR of a list of receivers (each a list of terms (node, comp, weight)): row_begin, cols, values = w phi rounded once
    (float64 product)."""
    rb, cols, vals = [0], [], []
    for terms in receivers:
        for node, comp, w in terms:
            cols.extend(term_columns(geom, node))
            vals.extend(np.float64(w) * term_values(geom, vecs, node, comp))
        rb.append(len(cols))
    return np.array(rb, dtype=np.uint32), np.array(cols, dtype=np.uint32), np.array(vals, dtype=np.float64)


def receiver_value(geom, vecs, terms, u):
    """(y, S_abs, m) of one receiver on the coarse vector u [NP s] in np.longdouble: y = sum_t w_t sum_(p,d) phi u, S_abs the
    same over absolute values, m the number of products (the rounding of w phi is one of the + 16 of the bar)."""
    u = np.asarray(u).astype(np.longdouble)
    y, sabs, m = np.longdouble(0), np.longdouble(0), 0
    for node, comp, w in terms:
        c = term_columns(geom, node)
        v = term_values(geom, vecs, node, comp).astype(np.longdouble) * np.longdouble(w)
        y += (v * u[c]).sum()
        sabs += (np.abs(v) * np.abs(u[c])).sum()
        m += len(c)
    return y, sabs, m


def point_terms(NE, x, y, comp=0):
    """The four bilinear terms of the point (x, y) of the unit square, written apart from slod_amd.point_terms: the element
    (ex, ey) that holds the point (the last one on the far boundary), nodes in the order (0,0), (1,0), (0,1), (1,1)."""
    NEp = NE + 1
    ex, ey = min(int(x * NE), NE - 1), min(int(y * NE), NE - 1)
    tx, ty = x * NE - ex, y * NE - ey
    return [(ex + ey * NEp, comp, (1 - tx) * (1 - ty)), (ex + 1 + ey * NEp, comp, tx * (1 - ty)),
            (ex + (ey + 1) * NEp, comp, (1 - tx) * ty), (ex + 1 + (ey + 1) * NEp, comp, tx * ty)]


def covering_patches(geom, node):
    """Number of patches whose closed extent holds the node, from the extents alone (no clipped centre range)."""
    n = geom.n
    X, Y = node % geom.NEp, node // geom.NEp
    e = geom.ext
    return int(((e[:, 0] * n <= X) & (X <= (e[:, 0] + e[:, 2]) * n) & (e[:, 1] * n <= Y) & (Y <= (e[:, 1] + e[:, 3]) * n)).sum())


def sample_nodes(geom, count=64, seed=5):
    """Fine nodes that hold the four domain corners, edge nodes, coarse-cell corners and cell-interior nodes, `count` in all
    (every node when the grid has no more)."""
    NEp, n, NE = geom.NEp, geom.n, geom.NE
    if NEp * NEp <= count:
        return np.arange(NEp * NEp)
    rng = np.random.default_rng(seed)
    picked = [0, NE, NE * NEp, NE * NEp + NE]
    mid = NE // 2
    picked += [mid, mid * NEp, mid * NEp + NE, NE * NEp + mid, 1, NEp]                                # edges
    picked += [n * (1 + i) + n * (1 + j) * NEp for i in range(min(3, geom.N - 1)) for j in range(min(3, geom.N - 1))]   # cell corners
    if n > 1:
        picked += [n * i + 1 + (n * j + 1) * NEp for i in range(min(3, geom.N)) for j in range(min(3, geom.N))]     # cell interiors
    rest = [k for k in rng.permutation(NEp * NEp) if k not in set(picked)]
    picked = list(dict.fromkeys(picked)) + [int(k) for k in rest]
    return np.array(picked[:count], dtype=np.int64)
