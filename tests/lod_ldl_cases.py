"""Helpers of the tests of the banded LDL^T factor (slod_lod_factor_create_ldl, slod_lod_factor_inertia) and of the
eigensolver near a shift (slod_lod_eigs_shift_direct); a plain module like lod_cases.py.

The yardstick is an unpivoted LDL^T in numpy float64 of the dense S, permuted to factor order: L, d, the inertia and
G = || |L| |D| |L^T| ||_inf.  Nothing in the yardstick, the shift rule or the surrogate pencil calls the library, so
test_lod_ldl_reference.py checks them on the CPU.

Bars (b = half bandwidth, u = 2^-53):
  inertia         n_negative equals the number of eigenvalues of scipy's eigh(sym A, M) below sigma, exactly
  norm_matrix     (2 b + 2) u relative: a row of the band has at most 2 b + 1 entries, summed in a fixed order
  norm_factor     a factor of 2 of the yardstick's G (what include/slod.h promises)
  backward error  eta = ||b - S x||_inf / (G ||x||_inf + ||b||_inf) <= (3 (b + 1) + 1) (b + 1) u, the residual in
                  np.longdouble and G from the yardstick: the project's Cholesky bound with ||A|| replaced by G, which
                  is what Higham, Accuracy and Stability, Thm 9.4 (elimination without pivoting, |dA| <= gamma_3k |L| |U|)
                  gives with U = D L^T
  growth          G / ||S||_inf <= 1e4 at every shift the rule accepts
"""
import numpy as np

U = 2.0 ** -53
GROWTH_CAP = 1e4
REL_GAP = 1e-6


class Ldl:
    pass


def ldl_reference(S):
    """Unpivoted LDL^T of the symmetric matrix whose lower triangle is that of S (already in factor order).  .bad is the
    index of the first pivot that is zero or not finite (-1: none; L, d and G are then complete)."""
    n = S.shape[0]
    W = np.tril(S) + np.tril(S, -1).T
    out = Ldl()
    out.L, out.d, out.bad = np.eye(n), np.zeros(n), -1
    with np.errstate(all="ignore"):
        for j in range(n):
            p = out.d[j] = W[j, j]
            if not (np.isfinite(p) and p != 0.0):
                out.bad = j
                break
            w = W[j + 1:, j].copy()
            out.L[j + 1:, j] = w / p
            W[j + 1:, j + 1:] -= np.outer(out.L[j + 1:, j], w)
    out.n_negative, out.n_positive = int((out.d < 0.0).sum()), int((out.d > 0.0).sum())
    aL = np.abs(out.L)
    out.G = float((aL @ (np.abs(out.d) * (aL.T @ np.ones(n)))).max()) if out.bad < 0 else float("nan")
    out.norm = float(np.abs(np.tril(S) + np.tril(S, -1).T).sum(axis=1).max())
    return out


def shift_at(lam, A, M, t, perm=None):
    """The first midpoint sigma of the gaps t, t + 1, .., t + 7 of the ascending spectrum lam of (A, M) (gap g lies
    between lam[g - 1] and lam[g]: g eigenvalues are below it) with a relative gap >= 1e-6, the yardstick's inertia equal
    to g and the yardstick's growth <= 1e4.  Returns (sigma, g, yardstick); none of the eight: AssertionError, with the
    growths that were measured."""
    perm = np.arange(len(lam)) if perm is None else perm
    seen = []
    for g in range(t, t + 8):
        if g < 1 or g >= len(lam):
            continue
        sigma = 0.5 * (lam[g - 1] + lam[g])
        if (lam[g] - lam[g - 1]) < REL_GAP * abs(sigma):
            seen.append((g, "gap"))
            continue
        S = (A - sigma * M)[np.ix_(perm, perm)]
        ref = ldl_reference(S)
        growth = ref.G / ref.norm
        seen.append((g, ref.n_negative, growth))
        if ref.bad < 0 and ref.n_negative == g and growth <= GROWTH_CAP:
            return float(sigma), g, ref
    raise AssertionError("no shift in the gaps %d .. %d qualifies: %r" % (t, t + 7, seen))


def five_shifts(lam, A, M, perm=None):
    """[(label, sigma, eigenvalues below sigma, yardstick)]: the rule at t = 1, rows // 4, rows // 2, then lambda_1 / 2
    (no negative pivot) and 2 lambda_max (all negative)."""
    rows = len(lam)
    perm = np.arange(rows) if perm is None else perm
    out = []
    for t in (1, rows // 4, rows // 2):
        sigma, g, ref = shift_at(lam, A, M, t, perm)
        out.append(("t=%d" % t, sigma, g, ref))
    for label, sigma, g in (("lambda_1/2", 0.5 * lam[0], 0), ("2 lambda_max", 2.0 * lam[-1], rows)):
        out.append((label, float(sigma), g, ldl_reference((A - sigma * M)[np.ix_(perm, perm)])))
    return out


def bound(b):
    return (3 * (b + 1) + 1) * (b + 1) * U


def eta(S, G, x, rhs):
    """Normwise backward error per column relative to G, the residual in extended precision."""
    r = rhs.astype(np.longdouble) - S.astype(np.longdouble) @ x.astype(np.longdouble)
    return np.array(np.abs(r).max(axis=0) / (G * np.abs(x).max(axis=0) + np.abs(rhs).max(axis=0)), dtype=np.float64)


def banded_solve(ref, rhs):
    """x = L^-T D^-1 L^-1 rhs with the yardstick's factor (scipy's triangular solves)."""
    import scipy.linalg as sl
    y = sl.solve_triangular(ref.L, rhs, lower=True, unit_diagonal=True)
    return sl.solve_triangular(ref.L.T, y / ref.d[:, None], lower=False, unit_diagonal=True)


def hash_block(nrow, m):
    """The start block of slod_lod_eigs_shift_direct with start = 0 (the formula of include/slod.h), [nrow][m]."""
    u = np.uint64
    i, j = np.meshgrid(np.arange(nrow, dtype=np.uint64), np.arange(m, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        z = (i << u(32) | j) + u(0x9E3779B97F4A7C15)
        z = (z ^ z >> u(30)) * u(0xBF58476D1CE4E5B9)
        z = (z ^ z >> u(27)) * u(0x94D049BB133111EB)
        z ^= z >> u(31)
    return (z >> u(11)).astype(np.float64) * 2.0 ** -52 - 1.0


# ---- the surrogate of the feasibility check: Q1 stiffness and mass on a square grid of nodes, random coefficient

def q1_pencil(inner, contrast=1e4, seed=20251020):
    """Q1 stiffness (one coefficient per cell, log-uniform in [1, contrast]) and mass on the inner x inner interior nodes
    of the unit square with a homogeneous Dirichlet boundary: (A, M) dense, nodes row-major (a band of half width
    inner + 1)."""
    nodes = inner + 2
    ne, h = nodes - 1, 1.0 / (nodes - 1)
    rng = np.random.default_rng(seed)
    coef = contrast ** rng.uniform(0.0, 1.0, (ne, ne))
    ke = np.array([[4, -1, -2, -1], [-1, 4, -1, -2], [-2, -1, 4, -1], [-1, -2, -1, 4]]) / 6.0
    me = np.array([[4, 2, 1, 2], [2, 4, 2, 1], [1, 2, 4, 2], [2, 1, 2, 4]]) * (h * h / 36.0)
    n = nodes * nodes
    A, M = np.zeros((n, n)), np.zeros((n, n))
    for ey in range(ne):
        for ex in range(ne):
            v = [ey * nodes + ex, ey * nodes + ex + 1, (ey + 1) * nodes + ex + 1, (ey + 1) * nodes + ex]
            A[np.ix_(v, v)] += coef[ey, ex] * ke
            M[np.ix_(v, v)] += me
    keep = np.array([y * nodes + x for y in range(1, nodes - 1) for x in range(1, nodes - 1)])
    return A[np.ix_(keep, keep)], M[np.ix_(keep, keep)]


# ---- the four cases of test_gpu_lod_factor.py with their real sym(A), M and the five shifts (needs a GPU)

CASES = ("dense", "rowmajor", "s2", "morton16")
_cases = {}


def factor_order(c):
    """perm[r] = the caller's row p s + d of factor index r = (cy N + cx) s + d."""
    g, s = c.g, c.s
    perm = np.zeros(c.nrow, dtype=np.int64)
    for p in range(g.num_patches):
        info = g.patch_layout(p)
        for d in range(s):
            perm[(info.cy * g.N + info.cx) * s + d] = p * s + d
    return perm


def ldl_case(so, name):
    """Handle, sym(A), M (device block rows and dense copies), the factor order, the half bandwidth, scipy's spectrum and
    the five shifts; built once.  dense: 16 rows, one tile; rowmajor: 25 rows, padding in n and b; s2: elasticity, 128
    rows; morton16: 256 rows, Morton ids; step64: 64 rows (the eigensolver tests)."""
    import scipy.linalg as sl
    from lod_cases import _build, _mass, _pencil, _rows_to_dense, _symmetrize
    if name not in _cases:
        if name in ("dense", "rowmajor", "step64"):
            c = _pencil(so, {"dense": "s1"}.get(name, name))
        else:
            c = _build(so, dict(nref=3, n_sub=2, oversampling=1, spacedim=2) if name == "s2"
                       else dict(nref=4, n_sub=2, oversampling=1, spacedim=1))
            c.mvalues, _ = _mass(c)
            c.sym = _symmetrize(c)
            hc = c.cols.cpu().numpy().view(np.uint32)
            c.A = _rows_to_dense(c.g, c.sym.cpu().numpy(), hc, c.s)
            c.M = _rows_to_dense(c.g, c.mvalues.cpu().numpy(), hc, c.s)
            assert np.array_equal(c.A, c.A.T) and np.array_equal(c.M, c.M.T)
            c.lam = sl.eigh(c.A, c.M, eigvals_only=True)
        c.perm = factor_order(c)
        w = 2 * c.g.cfg.oversampling + 1
        c.hbw = c.s * (w * c.g.N + w) + c.s - 1
        c.shifts = five_shifts(c.lam, c.A, c.M, c.perm)
        _cases[name] = c
    return _cases[name]


def shifted_values(c, sigma):
    """sym(A) - sigma M by slod_lod_matrix_combine on the device, and its dense copy (the words the factor reads)."""
    from lod_cases import NAN, _rows_to_dense, _torch
    torch, dev = _torch()
    out = torch.full_like(c.sym, NAN)
    c.g.lod_matrix_combine(1.0, c.sym.data_ptr(), -sigma, c.mvalues.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out, _rows_to_dense(c.g, out.cpu().numpy(), c.cols.cpu().numpy().view(np.uint32), c.s)


def diagonal_word(c, r=0):
    """The position in the block rows of the diagonal entry of factor index r."""
    row = int(c.perm[r])
    p, d = divmod(row, c.s)
    cap = c.g.lod_row_capacity()
    hc = c.cols.cpu().numpy().view(np.uint32).reshape(-1, cap)
    j = int(np.nonzero(hc[p] == p)[0][0])
    return (p * cap + j) * c.s * c.s + d * c.s + d
