"""Helpers of the tests of slod_lod_eigs_direct and slod_lod_eigs_ensemble_direct (a plain module like lod_cases.py):
the ensemble configurations of test_gpu_lod_ensemble_direct.py built once per session, shifted matrices and their
factors, single and ensemble calls with NaN-filled blocks, and the model of the outer iteration in numpy that the
tests use on the CPU to choose a tolerance or a case before anything runs on the device.  Nothing in the model calls
the library."""
import math

import numpy as np

from conftest import make_fields
from lod_cases import NAN, _bits, _lod_matrix, _rows_to_dense, _torch

DISTS = ("const", "D100", "D1e4")
CONFIGS = {"base": dict(nref=3, n_sub=2, oversampling=1, spacedim=1),      # 64 rows, the band is truncated
           "s2": dict(nref=3, n_sub=2, oversampling=1, spacedim=2),        # elasticity, 128 rows
           "rowmajor": dict(n_cells=5, n_sub=3, oversampling=1, spacedim=1)}   # 25 rows, padding in n and in b
ROWS = {"base": 64, "s2": 128, "rowmajor": 25}
NAMES = sorted(CONFIGS)
_cache = {}


class _Ens:
    pass


def _nan(*shape):
    torch, dev = _torch()
    return torch.full(shape, NAN, dtype=torch.float64, device=dev)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


# ---- the model: block inverse iteration with Rayleigh-Ritz in numpy / scipy

def outer_bound(rho, tol):
    """The project's bound on the outer iterations, 2 ceil(log tol / log rho) + 5 (test_gpu_lod_eig.py)."""
    return 5 if rho <= 0.0 else 2 * math.ceil(math.log(tol) / math.log(rho)) + 5


def contraction(lam, n_eig, m, sigma=0.0):
    """rho = (lambda_{n_eig} - sigma) / (lambda_{m+1} - sigma), lambda_{rows+1} = infinity."""
    return (lam[n_eig - 1] - sigma) / (lam[m] - sigma) if m < len(lam) else 0.0


def sine_block(g, s, m):
    """The start block of slod_lod_eigs (include/slod.h) in numpy, [num_patches * s][m]."""
    N = g.N
    side = min(N, 64)
    ab = sorted(((a, b) for a in range(1, side + 1) for b in range(1, side + 1)), key=lambda t: (t[0] ** 2 + t[1] ** 2, t[0]))
    X = np.zeros((g.num_patches * s, m))
    for p in range(g.num_patches):
        info = g.patch_layout(p)
        for j in range(m):
            a, b = ab[j // s]
            X[p * s + j % s, j] = math.sin(a * math.pi * (info.cx + 0.5) / N) * math.sin(b * math.pi * (info.cy + 0.5) / N)
    return X


def model_eigs(A, M, X, n_eig, tol, max_outer=200, sigma=0.0):
    """The outer iteration of include/slod.h on dense matrices: (theta, residuals, outer iterations, X)."""
    import scipy.linalg as sl
    S = A - sigma * M
    theta = res = None
    for outer in range(1, max_outer + 1):
        Z = np.linalg.solve(S, M @ X)
        W, V = A @ Z, M @ Z
        Ga, Gm = Z.T @ W, Z.T @ V
        theta, Q = sl.eigh(0.5 * (Ga + Ga.T), 0.5 * (Gm + Gm.T))
        X = Z @ Q
        AX, MX = W @ Q, V @ Q
        res = np.linalg.norm(AX - MX * theta, axis=0) / (np.abs(theta) * np.linalg.norm(MX, axis=0))
        if (res[:n_eig] <= tol).all():
            break
    return theta, res, outer, X


# ---- the ensemble configurations

def _single(c, call, *args):
    torch, dev = _torch()
    out = _nan(c.nval)
    call(*args, out.data_ptr())
    torch.cuda.synchronize()
    return out


def ensemble_case(so, name):
    """Handle with n_problems = 3 (members const / D100 / D1e4), the ensemble slab from one plan, and per member the
    single-problem A, sym(A) and M on the shared pattern, with dense copies; built once and left unchanged."""
    if name in _cache:
        return _cache[name]
    import slod_amd
    torch, dev = _torch()
    kw = CONFIGS[name]
    c = _Ens()
    c.name, c.s, c.K = name, kw["spacedim"], len(DISTS)
    cfg = so.make_cfg(stabilize=1, **kw)
    g = c.g = slod_amd.Slod(nref=kw.get("nref", 0), n_sub=kw["n_sub"], oversampling=kw["oversampling"], spacedim=c.s,
                            n_cells=kw.get("n_cells", 0), n_problems=c.K)
    for k, dist in enumerate(DISTS):
        for f, a in enumerate(make_fields(so, cfg, dist)):
            g.set_coefficient(f, a, problem=k)
    NP = c.NP = g.num_patches
    plan = g.plan(np.arange(c.K * NP, dtype=np.uint32))
    c.stride = plan.stride
    c.mstride = NP * c.stride
    c.b = torch.zeros(c.K * c.mstride, dtype=torch.float64, device=dev)
    c.q = torch.zeros_like(c.b)
    plan.execute(c.b.data_ptr(), c.q.data_ptr())
    plan.status()
    torch.cuda.synchronize()
    c.nrow, c.cap, c.field = NP * c.s, g.lod_row_capacity(), (g.NE + 1) ** 2 * c.s
    assert c.nrow == ROWS[name]
    c.nval = NP * c.cap * c.s * c.s
    c.slab = [(c.b[k * c.mstride:(k + 1) * c.mstride], c.q[k * c.mstride:(k + 1) * c.mstride]) for k in range(c.K)]
    c.values, c.cols = [], None
    for bk, qk in c.slab:
        v, cols = _lod_matrix(g, bk, qk, c.stride, c.s)
        c.values.append(v)
        assert c.cols is None or torch.equal(c.cols, cols)
        c.cols = cols
    c.hcols = c.cols.cpu().numpy().view(np.uint32)
    c.sym = [_single(c, g.lod_matrix_symmetrize, v.data_ptr(), c.cols.data_ptr()) for v in c.values]
    c.mass = []
    for k in range(c.K):
        mv = _nan(c.nval)
        mc = torch.zeros_like(c.cols)
        g.lod_mass_matrix(np.arange(NP), c.slab[k][0].data_ptr(), c.stride, mv.data_ptr(), mc.data_ptr())
        torch.cuda.synchronize()
        c.mass.append(mv)
    c.A = [dense(c, v) for v in c.sym]
    c.M = [dense(c, v) for v in c.mass]
    _cache[name] = c
    return c


def dense(c, values):
    return _rows_to_dense(c.g, values.contiguous().cpu().numpy(), c.hcols, c.s)


def stack(c, mats, K, pad=0):
    """K matrices interleaved [nval][K + pad], NaN in the padding: the three members, then (1 + k/64) member[k mod 3]."""
    torch, dev = _torch()
    f = [1.0 if k < c.K else 1.0 + k / 64.0 for k in range(K)]
    V = _nan(c.nval, K + pad)
    V[:, :K] = torch.stack([mats[k % c.K] * f[k] for k in range(K)], dim=1)
    return V


def shifted(g, cols, sym, mass, sigma):
    """sym(A) - sigma M by slod_lod_matrix_combine; sigma = 0 gives sym(A) itself (no call)."""
    if sigma == 0.0:
        return sym
    torch, dev = _torch()
    out = torch.full_like(sym, NAN)
    g.lod_matrix_combine(1.0, sym.data_ptr(), -sigma, mass.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out


# ---- the two calls on NaN-filled blocks

def eigs_direct(g, f, sym, mass, cols, nrow, n_eig, m, X0=None, ld=None, **kw):
    """slod_lod_eigs_direct; X0 (numpy [nrow][m]) makes start = 1.  Returns (lam, res, outer, X [nrow][ld])."""
    ld = m if ld is None else ld
    X = _nan(nrow, ld)
    if X0 is not None:
        X[:, :m] = _dev(X0)
    lam, res, outer = g.lod_eigs_direct(f, sym.data_ptr(), mass.data_ptr(), cols.data_ptr(), n_eig, X.data_ptr(), n_block=m,
                                        ld_x=ld, start=0 if X0 is None else 1, **kw)
    return lam, res, outer, X


def eigs_ensemble(g, f, A, M, cols, nrow, K, n_eig, m, X0=None, ld=None, ld_a_m=None, ld_m_m=None, **kw):
    """slod_lod_eigs_ensemble_direct; X0 (numpy [nrow][K m]) makes start = 1.  Returns (lam [K][m], res [K][m],
    member_status [K], rc, X [nrow][ld])."""
    ld = K * m if ld is None else ld
    X = _nan(nrow, ld)
    if X0 is not None:
        X[:, :K * m] = _dev(X0)
    lam, res, status, rc = g.lod_eigs_ensemble_direct(f, A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, n_eig, X.data_ptr(),
                                                      n_block=m, ld_a_m=ld_a_m, ld_m_m=ld_m_m, ld_x=ld,
                                                      start=0 if X0 is None else 1, **kw)
    return lam, res, status, rc, X


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def member_singles(c, A, M, K, n_eig, m, X0=None, **kw):
    """slod_lod_eigs_direct on every de-interleaved member of the ensemble matrices A, M [nval][>= K], on its single
    factor of A_k, from its own columns of X0: a list of (lam, res, outer, X bits [nrow][m])."""
    out = []
    for k in range(K):
        Ak, Mk = A[:, k].contiguous(), M[:, k].contiguous()
        fk = c.g.lod_factor(Ak.data_ptr(), c.cols.data_ptr())
        lam, res, outer, X = eigs_direct(c.g, fk, Ak, Mk, c.cols, c.nrow, n_eig, m,
                                         X0=None if X0 is None else X0[:, k * m:(k + 1) * m], **kw)
        out.append((lam, res, outer, _bits(X)))
        fk.close()
    return out
