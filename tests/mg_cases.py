"""The multigrid V-cycle of the FEM reference solves (csrc/slod_fem.hip: MgHierarchy, fem_solve_grid) restated with
scipy.sparse, in float64 and in numpy.longdouble, and the cases the tests of it share (a plain helper module like
lod_cases.py, not a conftest; nothing here calls the library or looks at a device result).

The algorithm, from the comments of the source and not from its kernels:
  levels    N_0 = NE, N_{l+1} = N_l / 2 while N_l is even and N_l / 2 >= 2
  transfer  bilinear P on the interior nodes (weights 1, 1/2, 1/4), restriction P^T, A_{l+1} = P^T A_l P
  smoother  x += omega_l D_l^-1 (b - A_l x), D_l the diagonal (s = 1) or the 2 x 2 node blocks (s = 2) of A_l,
            omega_l = min(0.8, 1.6 / ||D_l^-1 A_l||_inf): omega_l lambda_max(D_l^-1 A_l) <= 1.6 < 2 on every level
  cycle     V(2,2) from a zero start
  coarsest  2 sweeps with omega = 1 when N <= 2 (one interior node: exact), otherwise 40 damped sweeps
  driver    PCG with x_0 = 0 and the recursive residual, the stop test r.r <= tol^2 b.b once per burst of 4 steps

Unknowns are the interior dofs in (node, component) order, nodes lexicographic with x fastest: the order of
lod_cases._fem_reference, whose matrix is level 0.

The bar of every device comparison comes from the two references alone: e64 is the distance of the float64 from the
longdouble result for the same load and step, relative to max |reference|, and the bar is max(1e-13, 100 e64) (the
device sums the stencil entries with fma in another order than either reference)."""
import numpy as np
import scipy.sparse as sp

from conftest import SEED, make_fields
from lod_cases import _fem_reference

OMEGA_CAP, OMEGA_TARGET = 0.8, 1.6
NU, COARSEST_SWEEPS, BURST, JACOBI_BURST = 2, 40, 4, 32
FLOOR, FACTOR = 1e-13, 100.0
LD = np.longdouble

# (kind, NE of the solved grid, spacedim, field).  fine: slod_fem_solve on n_cells x n_sub = NE; coarse:
# slod_coarse_fem_solve on the n_cells = NE coarse cells of a fine grid with n_sub = 4
GEOMETRY = {4: (2, 2), 6: (3, 2), 8: (4, 2), 10: (5, 2), 12: (3, 4), 16: (4, 4)}      # NE -> (n_cells, n_sub)
DISTS = ("D100", "D1e4")
SCALAR = [("fine", NE, 1, d) for NE in (4, 6, 8, 10, 12, 16) for d in DISTS]
VECTOR = [("fine", NE, 2, d) for NE in (4, 6, 8, 12) for d in DISTS] + [("fine", 16, 2, "D1e4")]
COARSE = [("coarse", N, 1, d) for N in (8, 6) for d in DISTS]
CASES = SCALAR + VECTOR + COARSE
INDEFINITE_TODAY = [("fine", NE, 2, "D1e4") for NE in (8, 12, 16)]     # B is indefinite with a constant omega = 0.8
LONGDOUBLE_MAX_NE = 12
N_DENSE = 3


def case_id(case):
    return "%s-NE%d-s%d-%s" % case


def case_kw(case):
    kind, NE, s, _ = case
    n_cells, n_sub = GEOMETRY[NE] if kind == "fine" else (NE, 4)
    return dict(n_cells=n_cells, n_sub=n_sub, oversampling=1, spacedim=s, stabilize=1)


def coarse_field(field, N, n):
    """The field [NE][NE][4] at the 2 x 2 Gauss points of the N x N coarse cells, [N][N][4]: the coarse Gauss point
    reads the quadrature slot of the quadrant of the fine element it lies in (what slod_coarse_coefficient returns,
    pinned bit for bit by test_gpu_coarse_fem.py)."""
    NE = N * n
    g0 = 0.5 * (1.0 - 1.0 / np.sqrt(3.0))
    cy, cx, q = np.meshgrid(np.arange(N), np.arange(N), np.arange(4), indexing="ij")
    x = (cx + np.where(q & 1, 1.0 - g0, g0)) / N
    y = (cy + np.where(q & 2, 1.0 - g0, g0)) / N
    jx, jy = np.floor(2 * NE * x).astype(np.int64), np.floor(2 * NE * y).astype(np.int64)
    return np.asarray(field).reshape(NE, NE, 4)[jy // 2, jx // 2, (jx % 2) + 2 * (jy % 2)].ravel()


_fields, _problems, _hier, _bmat, _e64 = {}, {}, {}, {}, {}


def fields_of(so, case):
    """(fine fields handed to the handle, fields of the solved grid)."""
    if case not in _fields:
        kw = case_kw(case)
        fine = make_fields(so, so.make_cfg(**kw), case[3], SEED)
        solved = fine if case[0] == "fine" else [coarse_field(f, kw["n_cells"], kw["n_sub"]) for f in fine]
        _fields[case] = (fine, solved)
    return _fields[case]


def problem(so, case):
    """(A, idx): the float64 matrix of the interior dofs (csr) and their indices among all [(NE+1)^2][s] dofs."""
    if case not in _problems:
        A, _, idx = _fem_reference(case[1], case[2], fields_of(so, case)[1])
        _problems[case] = (sp.csr_matrix(A), idx)
    return _problems[case]


# ---- the hierarchy ----------------------------------------------------------------------------------------

def level_sizes(NE):
    out = [NE]
    while out[-1] % 2 == 0 and out[-1] // 2 >= 2:
        out.append(out[-1] // 2)
    return out


def _p1d(Nf, dtype):
    """1-D interpolation, interior fine nodes x interior coarse nodes."""
    Nc = Nf // 2
    P = np.zeros((Nf - 1, Nc - 1), dtype=dtype)
    for X in range(1, Nc):
        P[2 * X - 2, X - 1], P[2 * X - 1, X - 1], P[2 * X, X - 1] = 0.5, 1.0, 0.5
    return P


def p1d_all_nodes(Nf):
    """The same interpolation on every node, the rim included: (Nf + 1) x (Nc + 1)."""
    Nc = Nf // 2
    P = np.zeros((Nf + 1, Nc + 1))
    for X in range(Nc + 1):
        for f in (2 * X - 1, 2 * X, 2 * X + 1):
            if 0 <= f <= Nf:
                P[f, X] = 1.0 if f == 2 * X else 0.5
    return P


def _transfer(Nf, s, dtype, r1d=None):
    p = _p1d(Nf, dtype) if r1d is None else r1d
    return sp.csr_matrix(sp.kron(sp.kron(sp.csr_matrix(p), sp.csr_matrix(p)), sp.identity(s, dtype=dtype)), dtype=dtype)


def _block_inverse(A, s, dtype, point=False):
    """D^-1 as a sparse matrix: D the diagonal, or the 2 x 2 node blocks, of A."""
    d = A.diagonal().astype(dtype)
    n = d.size
    if s == 1 or point:
        return sp.diags(1.0 / d).tocsr().astype(dtype)
    up, lo = A.diagonal(1).astype(dtype)[::2], A.diagonal(-1).astype(dtype)[::2]
    d0, d1 = d[0::2], d[1::2]
    det = d0 * d1 - up * lo
    i0, i1 = np.arange(0, n, 2), np.arange(1, n, 2)
    rows = np.concatenate([i0, i0, i1, i1])
    cols = np.concatenate([i0, i1, i0, i1])
    vals = np.concatenate([d1 / det, -up / det, -lo / det, d0 / det])
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n), dtype=dtype)


def _swap_ab(A):
    """Every 2 x 2 block that couples two different nodes transposed (the stand-in of a Galerkin kernel that writes
    plane (dir, b, a) where (dir, a, b) belongs, off the centre)."""
    C = A.tocoo()
    ni, nj, a, b = C.row // 2, C.col // 2, C.row % 2, C.col % 2
    off = ni != nj
    rows = np.where(off, 2 * ni + b, C.row)
    cols = np.where(off, 2 * nj + a, C.col)
    return sp.csr_matrix((C.data, (rows, cols)), shape=A.shape, dtype=A.dtype)


MUTANTS = ("restrict_rim_weight", "galerkin_ab_swapped", "point_jacobi", "omega_on_N2", "missing_post_sweep")


class Hierarchy:
    """omega: "rule" (omega_l above) or a constant; mutant: one of MUTANTS, a reference with one mistake built in."""

    def __init__(self, A, NE, s, dtype=np.float64, omega="rule", mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.s, self.dtype, self.mutant = s, dtype, mutant
        self.post = 1 if mutant == "missing_post_sweep" else NU
        self.lev = []
        A = sp.csr_matrix(A, dtype=dtype)
        sizes = level_sizes(NE)
        for l, N in enumerate(sizes):
            L = dict(N=N, A=A, Dinv=_block_inverse(A, s, dtype, point=mutant == "point_jacobi"))
            M = L["Dinv"] @ A
            L["norm_inf"] = abs(M).sum(axis=1).max()
            L["omega"] = dtype(min(OMEGA_CAP, OMEGA_TARGET / float(L["norm_inf"])) if omega == "rule" else omega)
            if l + 1 < len(sizes):
                L["P"] = _transfer(N, s, dtype)
                L["R"] = L["P"].T.tocsr()
                if mutant == "restrict_rim_weight":      # the fine line next to the rim counted twice
                    r = _p1d(N, dtype)
                    r[0, 0] = r[-1, -1] = 1.0
                    L["R"] = _transfer(N, s, dtype, r).T.tocsr()
                A = sp.csr_matrix(L["P"].T @ A @ L["P"], dtype=dtype)
                if mutant == "galerkin_ab_swapped" and s == 2:
                    A = _swap_ab(A)
            self.lev.append(L)

    def lambda_max(self):
        """lambda_max(D_l^-1 A_l) per level (dense; for printing and for the CPU tests)."""
        out = []
        for L in self.lev:
            M = (L["Dinv"] @ L["A"]).toarray().astype(np.float64)
            out.append(float(np.linalg.eigvals(M).real.max()))
        return out

    def cycle(self, b, l=0):
        """One V-cycle on A_l x = b from x = 0; b a vector or a matrix of columns."""
        L, one = self.lev[l], self.dtype(1)
        last = l + 1 == len(self.lev)
        A, Dinv, om = L["A"], L["Dinv"], L["omega"]
        sweeps = NU
        if last:
            sweeps = 2 if L["N"] <= 2 else COARSEST_SWEEPS
            if L["N"] <= 2 and self.mutant != "omega_on_N2":
                om = one
        x = om * (Dinv @ b)
        for _ in range(1, sweeps):
            x = x + om * (Dinv @ (b - A @ x))
        if last:
            return x
        x = x + L["P"] @ self.cycle(L["R"] @ (b - A @ x), l + 1)
        for _ in range(self.post):
            x = x + om * (Dinv @ (b - A @ x))
        return x

    def matrix(self):
        n = self.lev[0]["A"].shape[0]
        return self.cycle(np.eye(n, dtype=self.dtype))


def hierarchy(so, case, dtype=np.float64, omega="rule", mutant=None):
    key = (case, np.dtype(dtype).name, omega, mutant)
    if key not in _hier:
        A, _ = problem(so, case)
        _hier[key] = Hierarchy(A, case[1], case[2], dtype, omega, mutant)
    return _hier[key]


def b_matrix(so, case, dtype=np.float64, omega="rule", mutant=None):
    """The V-cycle as a dense matrix B (read-only)."""
    key = (case, np.dtype(dtype).name, omega, mutant)
    if key not in _bmat:
        B = hierarchy(so, case, dtype, omega, mutant).matrix()
        B.setflags(write=False)
        _bmat[key] = B
    return _bmat[key]


# ---- the driver -------------------------------------------------------------------------------------------

def first_step(A, B, F):
    """u_1 = alpha B f, alpha = f.Bf / (Bf . A Bf), for every column f of F (what one PCG step from x_0 = 0 returns)."""
    Z = B @ F
    num = (F * Z).sum(axis=0)
    den = (Z * (A @ Z)).sum(axis=0)
    return Z * (num / den)


def first_step_unit(A, B):
    """first_step for every unit load at once: column j is u_1 of f = e_j."""
    num = np.diagonal(B)
    den = (B * (A @ B)).sum(axis=0)
    return B * (num / den)


def pcg(A, prec, f, max_iterations, tol=0.0, burst=BURST):
    """The recurrences of slod_cg_drive.  Returns (iterates [x_1, x_2, ...], relative residuals after every step, it)."""
    dtype = f.dtype
    A = A.astype(dtype)
    x, r = np.zeros_like(f), f.copy()
    z = prec(r)
    p, rz = z.copy(), r @ z
    rhs2 = rr = f @ f
    xs, res, it = [], [], 0
    while it < max_iterations and rhs2 > 0 and rr > dtype.type(tol) ** 2 * rhs2:
        for _ in range(min(burst, max_iterations - it)):
            Ap = A @ p
            alpha = rz / (p @ Ap)
            x = x + alpha * p
            r = r - alpha * Ap
            rr = r @ r
            z = prec(r)
            rz_new = r @ z
            p = z + (rz_new / rz) * p
            rz = rz_new
            it += 1
            xs.append(x)
            res.append(float(np.sqrt(rr / rhs2)))
    return xs, res, it


def jacobi_prec(A):
    dinv = 1.0 / A.diagonal()
    return lambda r: dinv * r


# ---- loads and bars ---------------------------------------------------------------------------------------

def dense_loads(so, case):
    """N_DENSE seeded uniform(-1, 1) loads on the interior dofs, columns of [n][N_DENSE]."""
    n = problem(so, case)[0].shape[0]
    return np.random.default_rng([SEED, CASES.index(case)]).uniform(-1.0, 1.0, (n, N_DENSE))


def unit_load_dofs(so, case):
    """The interior dofs (positions in the interior order) that get a unit load: all of them up to NE = 12; at NE = 16
    every node within two lines of the rim, the centre node and 16 seeded others, each with all its components."""
    _, NE, s, _ = case
    m = NE - 1
    if NE <= LONGDOUBLE_MAX_NE:
        return np.arange(m * m * s)
    iy, ix = np.divmod(np.arange(m * m), m)      # interior position; the node is (ix + 1, iy + 1)
    near = (np.minimum(ix, m - 1 - ix) < 2) | (np.minimum(iy, m - 1 - iy) < 2)
    nodes = set(np.nonzero(near)[0].tolist()) | {(NE // 2 - 1) * m + NE // 2 - 1}
    rest = np.array(sorted(set(range(m * m)) - nodes))
    nodes |= set(np.random.default_rng(SEED).choice(rest, 16, replace=False).tolist())
    return np.array([nd * s + c for nd in sorted(nodes) for c in range(s)])


def rel_dist(a, b):
    """max |a - b| / max |b| per column."""
    return np.abs(a - b).max(axis=0).astype(np.float64) / np.abs(b).max(axis=0).astype(np.float64)


def reference_u1(so, case, omega="rule"):
    """dict(unit, dense: float64 references of u_1 for the unit loads of unit_load_dofs and the dense loads;
    e64_unit, e64_dense: their distance from the longdouble reference per load, None when there is none)."""
    key = (case, "u1", omega)
    if key not in _e64:
        A, _ = problem(so, case)
        dofs, F = unit_load_dofs(so, case), dense_loads(so, case)
        B = b_matrix(so, case, omega=omega)
        out = dict(unit=first_step_unit(A, B)[:, dofs], dense=first_step(A, B, F), e64_unit=None, e64_dense=None)
        if case[1] <= LONGDOUBLE_MAX_NE:
            Aq, Bq = A.astype(LD), b_matrix(so, case, LD, omega)
            out["e64_unit"] = rel_dist(out["unit"], first_step_unit(Aq, Bq)[:, dofs])
            out["e64_dense"] = rel_dist(out["dense"], first_step(Aq, Bq, F.astype(LD)))
        _e64[key] = out
    return _e64[key]


TRAJECTORY_STEPS = (2, 3, 5, 8)


def reference_trajectory(so, case, omega="rule"):
    """u_k for k in TRAJECTORY_STEPS on dense load 0: (float64 references {k: u_k}, {k: e64} or None)."""
    key = (case, "traj", omega)
    if key not in _e64:
        A, _ = problem(so, case)
        f = dense_loads(so, case)[:, 0].copy()
        xs, _, _ = pcg(A, hierarchy(so, case, omega=omega).cycle, f, max(TRAJECTORY_STEPS))
        ref, e = {k: xs[k - 1] for k in TRAJECTORY_STEPS}, None
        if case[1] <= LONGDOUBLE_MAX_NE:
            xq, _, _ = pcg(A, hierarchy(so, case, LD, omega).cycle, f.astype(LD), max(TRAJECTORY_STEPS))
            e = {k: float(rel_dist(ref[k][:, None], xq[k - 1][:, None])[0]) for k in TRAJECTORY_STEPS}
        _e64[key] = (ref, e)
    return _e64[key]


def largest_small_e64(so, what):
    """The largest e64 over the cases that have a longdouble reference (what: "u1" or "traj"): the e64 of NE = 16."""
    worst = 0.0
    for case in CASES:
        if case[1] > LONGDOUBLE_MAX_NE:
            continue
        if what == "u1":
            r = reference_u1(so, case)
            worst = max(worst, float(r["e64_unit"].max()), float(r["e64_dense"].max()))
        else:
            worst = max(worst, max(reference_trajectory(so, case)[1].values()))
    return worst


def bar(e64):
    return np.maximum(FLOOR, FACTOR * np.asarray(e64))


# ---- the iteration count: a load on which one burst decides ------------------------------------------------

COUNT_MODES = 10
TOL_CANDIDATES = tuple(10.0 ** -e for e in range(5, 12))


def count_case(so, case):
    """(f, tol, expected iterations, residuals at the multiples of 4) for the iteration-count test.  A generic load
    loses about a digit per burst, so some burst always ends within a factor 10 of any tol.  The load here is A times
    a sum of COUNT_MODES eigenvectors of B A spread over its spectrum: PCG ends after COUNT_MODES steps in exact
    arithmetic, the residual falls by many digits inside one burst, and tol is the first of TOL_CANDIDATES from which
    every burst end of the float64 reference keeps a factor 10 (None when there is none)."""
    key = (case, "count")
    if key not in _e64:
        import scipy.linalg as sl
        A, _ = problem(so, case)
        B = b_matrix(so, case)
        Lc = np.linalg.cholesky(0.5 * (B + B.T))
        lam, W = sl.eigh(Lc.T @ (A @ Lc))
        n = lam.size
        pick = np.unique(np.round(np.linspace(0, n - 1, min(COUNT_MODES, n))).astype(int))
        V = Lc @ W[:, pick]
        V = V / np.abs(V).max(axis=0)
        f = A @ V.sum(axis=1)
        f = f / np.abs(f).max()
        _, res, _ = pcg(A, hierarchy(so, case).cycle, f, 24)
        ends = np.array(res[BURST - 1::BURST])
        tol = next((t for t in TOL_CANDIDATES if not ((ends >= t / 10) & (ends <= 10 * t)).any() and (ends < t).any()), None)
        expected = None if tol is None else BURST * (1 + int(np.argmax(ends < tol)))
        _e64[key] = (f, tol, expected, ends)
    return _e64[key]


# ---- naming a node in a failure message -------------------------------------------------------------------

def describe_dof(case, dof):
    """Node and component of an interior dof, the coarsest level on which the node is a grid node, and the nodes of
    the coarsest level whose (composite) hat covers it."""
    _, NE, s, _ = case
    m = NE - 1
    nd, c = divmod(int(dof), s)
    ix, iy = nd % m + 1, nd // m + 1
    sizes = level_sizes(NE)
    own = max(l for l in range(len(sizes)) if ix % (1 << l) == 0 and iy % (1 << l) == 0)
    st = 1 << (len(sizes) - 1)
    hats = [(X, Y) for Y in range(1, sizes[-1]) for X in range(1, sizes[-1]) if abs(ix - X * st) < st and abs(iy - Y * st) < st]
    return "node (%d, %d) component %d: a grid node down to level %d (N = %d); covered on the coarsest level %d (N = %d) " \
           "by the hats of %s" % (ix, iy, c, own, sizes[own], len(sizes) - 1, sizes[-1], hats)


# ---- the 65^2 elasticity grid of test_fem_multigrid_preconditioner -----------------------------------------

# Iterations the float64 reference needs at rel_tol 1e-12 on nref = 4, n_sub = 4, spacedim = 2, D1e4, f = 1 (multigrid
# in bursts of 4, Jacobi in bursts of 32); test_mg_reference.py recomputes them, the GPU test takes its ratio from them
PREDICTED_65 = dict(mg=104, jacobi=1376)


def predict_65(so, omega="rule"):
    """(multigrid iterations, Jacobi iterations) of the reference on that grid."""
    if "65" not in _problems:
        kw = dict(nref=4, n_sub=4, oversampling=1, spacedim=2, stabilize=1)
        A, f, _ = _fem_reference(64, 2, make_fields(so, so.make_cfg(**kw), "D1e4", SEED))
        _problems["65"] = (sp.csr_matrix(A), f)
    A, f = _problems["65"]
    _, _, it_mg = pcg(A, Hierarchy(A, 64, 2, omega=omega).cycle, f, 20000, 1e-12)
    _, _, it_j = pcg(A, jacobi_prec(A), f, 20000, 1e-12, burst=JACOBI_BURST)
    return it_mg, it_j
