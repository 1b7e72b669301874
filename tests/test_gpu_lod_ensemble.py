"""The ensemble block on the GPU: every member's matrix, load, product, solve and reconstruction has the bits of the
single-problem call on that member's slab, whatever n_members, the leading dimensions and the member's position; the
moments have the bits of the float64 loop.

One handle per configuration with n_problems = 3, members const / D100 / D1e4 of make_fields, one plan over all
3 * num_patches gids.  The single-problem references are computed once per configuration and shared."""
import numpy as np
import pytest

from conftest import make_fields
from lod_cases import NAN, _bits, _lod_matrix, _rows_to_dense, _torch

pytestmark = pytest.mark.gpu

DISTS = ("const", "D100", "D1e4")
CONFIGS = {"base": dict(nref=3, n_sub=2, oversampling=1, spacedim=1),      # 64 rows
           "s2": dict(nref=3, n_sub=2, oversampling=1, spacedim=2),
           "rowmajor": dict(n_cells=5, n_sub=3, oversampling=1, spacedim=1),
           "clipped": dict(nref=2, n_sub=4, oversampling=2, spacedim=1)}
NAMES = sorted(CONFIGS)
TOL = 1e-10
_cache = {}


class _Ens:
    pass


def _nan(*shape):
    torch, dev = _torch()
    return torch.full(shape, NAN, dtype=torch.float64, device=dev)


def _case(so, name):
    """Handle, ensemble slab, and per member the single-problem matrix, load vector (f = 1) and solve; built once."""
    if name in _cache:
        return _cache[name]
    import slod_amd
    torch, dev = _torch()
    kw = CONFIGS[name]
    c = _Ens()
    c.s, c.K = kw["spacedim"], len(DISTS)
    cfg = so.make_cfg(stabilize=1, **kw)
    g = c.g = slod_amd.Slod(nref=kw.get("nref", 0), n_sub=kw["n_sub"], oversampling=kw["oversampling"], spacedim=c.s,
                            n_cells=kw.get("n_cells", 0), n_problems=c.K)
    for k, dist in enumerate(DISTS):
        for f, a in enumerate(make_fields(so, cfg, dist)):
            g.set_coefficient(f, a, problem=k)
    NP = c.NP = g.num_patches
    plan = g.plan(np.arange(c.K * NP, dtype=np.uint32))              # one plan over all members
    c.stride = plan.stride
    c.mstride = NP * c.stride
    c.b = torch.zeros(c.K * c.mstride, dtype=torch.float64, device=dev)
    c.q = torch.zeros_like(c.b)
    plan.execute(c.b.data_ptr(), c.q.data_ptr())
    plan.status()
    torch.cuda.synchronize()
    c.nrow, c.cap, c.field = NP * c.s, g.lod_row_capacity(), (g.NE + 1) ** 2 * c.s
    c.nval = NP * c.cap * c.s * c.s
    c.slab = [(c.b[k * c.mstride:(k + 1) * c.mstride], c.q[k * c.mstride:(k + 1) * c.mstride]) for k in range(c.K)]
    c.values, c.cols = [], None
    for bk, qk in c.slab:
        v, cols = _lod_matrix(g, bk, qk, c.stride, c.s)
        c.values.append(v)
        assert c.cols is None or torch.equal(c.cols, cols)
        c.cols = cols
    c.load = torch.zeros(c.field, dtype=torch.float64, device=dev)
    g.fem_rhs(None, c.load.data_ptr())
    torch.cuda.synchronize()
    c.rhs = [_single_rhs(c, k, c.load) for k in range(c.K)]
    c.sol = [_single_solve(c, c.values[k], c.rhs[k]) for k in range(c.K)]
    _cache[name] = c
    return c


def _single_rhs(c, k, load):
    torch, dev = _torch()
    out = _nan(c.nrow)
    c.g.lod_rhs(np.arange(c.NP), c.slab[k][0].data_ptr(), c.stride, load.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out


def _single_solve(c, values, rhs, max_iterations=2000):
    """slod_lod_solve_multi(n_rhs = 1) on one de-interleaved member: (u, iterations, residual)"""
    torch, dev = _torch()
    values, rhs = values.contiguous(), rhs.contiguous()
    u = _nan(c.nrow)
    torch.cuda.synchronize()
    its, res = c.g.lod_solve_multi(values.data_ptr(), c.cols.data_ptr(), rhs.data_ptr(), 1, 1, u.data_ptr(), 1, rel_tol=TOL,
                                   max_iterations=max_iterations)
    return u, int(its[0]), float(res[0])


def _single_reconstruct(c, k, u):
    torch, dev = _torch()
    u = u.contiguous()
    fine = _nan(c.field)
    torch.cuda.synchronize()
    c.g.lod_reconstruct(c.slab[k][0].data_ptr(), c.stride, u.data_ptr(), fine.data_ptr())
    torch.cuda.synchronize()
    return fine


def _members(c, K):
    """K matrices and loads on the device: the three members, then scaled copies (1 + k/64) A_{k mod 3}; values
    interleaved [nval][K], rhs [nrow][K]."""
    torch, dev = _torch()
    f = [1.0 if k < c.K else 1.0 + k / 64.0 for k in range(K)]
    V = torch.stack([c.values[k % c.K] * f[k] for k in range(K)], dim=1).contiguous()
    R = torch.stack([c.rhs[k % c.K] for k in range(K)], dim=1).contiguous()
    return V, R


def _solve_ens(c, V, R, K, pad=2, max_iterations=2000):
    torch, dev = _torch()
    U = _nan(c.nrow, K + pad)
    torch.cuda.synchronize()
    its, res = c.g.lod_solve_ensemble(V.data_ptr(), c.cols.data_ptr(), R.data_ptr(), U.data_ptr(), K, ld_m=V.shape[1],
                                      ld_rhs=R.shape[1], ld_u=K + pad, rel_tol=TOL, max_iterations=max_iterations)
    return U, its.copy(), res.copy()


def _moments_numpy(x):
    """the obvious float64 loop: x [K][n]"""
    K = x.shape[0]
    total = x[0].copy()
    for k in range(1, K):
        total = total + x[k]
    mean = total / np.float64(K)
    acc = np.zeros_like(mean)
    for k in range(K):
        d = x[k] - mean
        acc = acc + d * d
    return mean, acc / np.float64(K - 1) if K > 1 else np.zeros_like(mean)


# ---- matrix

@pytest.mark.parametrize("name", NAMES)
def test_matrix_ensemble_equals_single_calls(so, name):
    torch, dev = _torch()
    c = _case(so, name)
    ld = c.K + 2
    V = _nan(c.nval, ld)
    cols = torch.full((c.NP * c.cap,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    c.g.lod_matrix_ensemble(c.b.data_ptr(), c.q.data_ptr(), c.stride, c.K, V.data_ptr(), cols.data_ptr(), ld_m=ld)
    torch.cuda.synchronize()
    for k in range(c.K):
        assert np.array_equal(_bits(V[:, k]), _bits(c.values[k])), (name, k)
    assert torch.equal(cols, c.cols)
    assert torch.isnan(V[:, c.K:]).all()
    # the members differ: the check above is not three times the same matrix
    assert not torch.equal(c.values[0], c.values[1]) and not torch.equal(c.values[1], c.values[2])
    # a member sub-range: base + first member of the slab and of the values
    W = _nan(c.nval, ld)
    c.g.lod_matrix_ensemble(c.b.data_ptr() + 8 * c.mstride, c.q.data_ptr() + 8 * c.mstride, c.stride, c.K - 1,
                            W.data_ptr() + 8, cols.data_ptr(), ld_m=ld)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(W[:, 1:c.K]), _bits(V[:, 1:c.K]))
    assert torch.isnan(W[:, 0]).all() and torch.isnan(W[:, c.K:]).all()


# ---- load vector and reconstruction

@pytest.mark.parametrize("shared", [True, False], ids=["shared_load", "distinct_loads"])
@pytest.mark.parametrize("name", NAMES)
def test_rhs_and_reconstruct_ensemble_equal_single_calls(so, name, shared):
    torch, dev = _torch()
    c = _case(so, name)
    gen = torch.Generator(device="cpu").manual_seed(11)
    ld_fine = c.field + 5
    if shared:
        loads = c.load
    else:
        loads = _nan(c.K, ld_fine)
        loads[:, :c.field] = (torch.rand(c.K, c.field, generator=gen, dtype=torch.float64) - 0.5).to(dev)
    out = _nan(c.nrow, c.K + 1)
    torch.cuda.synchronize()
    c.g.lod_rhs_ensemble(c.b.data_ptr(), c.stride, c.K, loads.data_ptr(), out.data_ptr(), ld_fine=0 if shared else ld_fine,
                         ld_out=c.K + 1)
    torch.cuda.synchronize()
    for k in range(c.K):
        ref = c.rhs[k] if shared else _single_rhs(c, k, loads[k, :c.field].contiguous())
        assert np.array_equal(_bits(out[:, k]), _bits(ref)), (name, k)
    assert torch.isnan(out[:, c.K]).all()
    # reconstruction of coarse vectors of their own per member
    U = _nan(c.nrow, c.K + 1)
    U[:, :c.K] = (torch.rand(c.nrow, c.K, generator=gen, dtype=torch.float64) - 0.5).to(dev)
    fine = _nan(c.K, ld_fine)
    torch.cuda.synchronize()
    c.g.lod_reconstruct_ensemble(c.b.data_ptr(), c.stride, c.K, U.data_ptr(), fine.data_ptr(), ld_fine=ld_fine, ld_u=c.K + 1)
    torch.cuda.synchronize()
    for k in range(c.K):
        assert np.array_equal(_bits(fine[k, :c.field]), _bits(_single_reconstruct(c, k, U[:, k]))), (name, k)
    assert torch.isnan(fine[:, c.field:]).all()


# ---- product

def _apply_ens(g, V, cols, X, Y, K, first=0):
    torch, dev = _torch()
    torch.cuda.synchronize()
    g.lod_apply_ensemble(V.data_ptr() + 8 * first, cols.data_ptr(), X.data_ptr() + 8 * first, Y.data_ptr() + 8 * first, K,
                         ld_m=V.shape[1], ld_x=X.shape[1], ld_y=Y.shape[1])
    torch.cuda.synchronize()


def _apply_single(g, values, cols, X, k, nrow):
    """slod_lod_apply_multi with n_rhs = 1 on column k of X and one de-interleaved matrix"""
    torch, dev = _torch()
    values = values.contiguous()
    y = _nan(nrow)
    torch.cuda.synchronize()
    g.lod_apply(values.data_ptr(), cols.data_ptr(), X.data_ptr() + 8 * k, y.data_ptr(), n_rhs=1, ld_x=X.shape[1], ld_y=1)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("K", [1, 3, 65])
@pytest.mark.parametrize("name", NAMES)
def test_apply_ensemble_equals_apply_multi(so, name, K):
    torch, dev = _torch()
    c = _case(so, name)
    V, _ = _members(c, K)
    gen = torch.Generator(device="cpu").manual_seed(5)
    X = _nan(c.nrow, K + 3)                                          # padded ld_x, ld_y
    X[:, :K] = (torch.rand(c.nrow, K, generator=gen, dtype=torch.float64) - 0.5).to(dev)
    Y = _nan(c.nrow, K + 1)
    _apply_ens(c.g, V, c.cols, X, Y, K)
    for k in range(K):
        assert np.array_equal(_bits(Y[:, k]), _bits(_apply_single(c.g, V[:, k], c.cols, X, k, c.nrow))), (name, K, k)
    assert torch.isnan(Y[:, K]).all()
    if K > 1:                                                        # a member sub-range: base pointers + first member
        first = K // 2
        Z = _nan(c.nrow, K + 1)
        _apply_ens(c.g, V, c.cols, X, Z, K - first, first=first)
        assert np.array_equal(_bits(Z[:, first:K]), _bits(Y[:, first:K]))
        assert torch.isnan(Z[:, :first]).all() and torch.isnan(Z[:, K]).all()


def test_apply_ensemble_walks_several_row_groups():
    """32768 rows are 2048 row groups for at most 1024 blocks per chunk: a block takes two.  A diagonal pattern needs no
    basis; every member has a diagonal of its own."""
    import slod_amd
    torch, dev = _torch()
    g = slod_amd.Slod(nref=7, n_sub=1, oversampling=1, spacedim=2)
    NP, cap, s, K = g.num_patches, g.lod_row_capacity(), 2, 3
    nrow = NP * s
    assert nrow == 32768
    cols = np.full((NP, cap), 0xffffffff, dtype=np.uint32)
    cols[:, 0] = np.arange(NP)
    ct = torch.from_numpy(cols.view(np.int32)).to(dev)
    gen = torch.Generator(device="cpu").manual_seed(3)
    diag = (torch.rand(nrow, K, generator=gen, dtype=torch.float64) + 0.5).to(dev)
    V5 = torch.zeros(NP, cap, s, s, K, dtype=torch.float64, device=dev)
    for d in range(s):
        V5[:, 0, d, d, :] = diag[d::s]
    V = V5.reshape(-1, K)
    X = (torch.rand(nrow, K, generator=gen, dtype=torch.float64) - 0.5).to(dev)
    Y = _nan(nrow, K)
    _apply_ens(g, V, ct, X, Y, K)
    # fma(a, x, 0) is the rounded product
    assert np.array_equal(_bits(Y), _bits(diag * X))
    k = 1
    assert np.array_equal(_bits(Y[:, k]), _bits(_apply_single(g, V[:, k], ct, X, k, nrow)))


# ---- solve

@pytest.mark.parametrize("K", [3, 65])
@pytest.mark.parametrize("name", NAMES)
def test_solve_ensemble_equals_single_solves(so, name, K):
    torch, dev = _torch()
    c = _case(so, name)
    V, R = _members(c, K)
    U, its, res = _solve_ens(c, V, R, K)
    for k in range(K):
        u, it, rs = c.sol[k] if k < c.K else _single_solve(c, V[:, k], R[:, k])
        assert np.array_equal(_bits(U[:, k]), _bits(u)), (name, K, k)
        assert its[k] == it, (name, K, k, its[k], it)
        assert np.float64(res[k]).view(np.uint64) == np.float64(rs).view(np.uint64), (name, K, k)
    assert torch.isnan(U[:, K:]).all()
    print("%s K=%d iterations %s" % (name, K, its[:c.K].tolist()))
    if name == "base":
        assert len(set(its[:c.K].tolist())) > 1, "the members freeze at the same check: %s" % its[:c.K]


@pytest.mark.parametrize("name", NAMES)
def test_solve_ensemble_properties(so, name):
    torch, dev = _torch()
    c = _case(so, name)
    K = c.K
    V, R = _members(c, K)
    U, its, res = _solve_ens(c, V, R, K)
    hcols = c.cols.cpu().numpy().view(np.uint32)
    # against the dense solve of every member
    for k in range(K):
        A = _rows_to_dense(c.g, c.values[k].cpu().numpy(), hcols, c.s)
        ref = np.linalg.solve(A, c.rhs[k].cpu().numpy())
        err = np.abs(U[:, k].cpu().numpy() - ref).max() / np.abs(ref).max()
        print("%s member %d: %d iterations, residual %.3e, error against the dense solve %.3e" % (name, k, its[k], res[k], err))
        assert err <= 1e-8, (name, k, err)
    # a repeated call repeats the bits
    U2, its2, res2 = _solve_ens(c, V, R, K)
    assert np.array_equal(_bits(U2[:, :K]), _bits(U[:, :K])) and np.array_equal(its2, its)
    assert np.array_equal(res2.view(np.uint64), res.view(np.uint64))
    # a permutation of the members permutes the results
    perm = [2, 0, 1]
    Up, itsp, resp = _solve_ens(c, V[:, perm].contiguous(), R[:, perm].contiguous(), K, pad=0)
    assert np.array_equal(_bits(Up), _bits(U[:, perm])) and np.array_equal(itsp, its[perm])
    assert np.array_equal(resp.view(np.uint64), res[perm].view(np.uint64))
    # a zero member is done at once and the others run on
    Rz = R.clone()
    Rz[:, 1] = 0.0
    Uz, itsz, resz = _solve_ens(c, V, Rz, K)
    assert (Uz[:, 1] == 0.0).all() and itsz[1] == 0 and resz[1] == 0.0
    for k in (0, 2):
        assert np.array_equal(_bits(Uz[:, k]), _bits(U[:, k])) and itsz[k] == its[k]
    assert torch.isnan(Uz[:, K:]).all()
    # max_iterations = 8 stops every unconverged member at 8, without error
    U8, its8, res8 = _solve_ens(c, V, R, K, max_iterations=8)
    for k in range(K):
        assert its8[k] == min(8, its[k]), (name, k, its8, its)
        if its[k] > 8:
            assert res8[k] > TOL
        u, it, rs = _single_solve(c, V[:, k], R[:, k], max_iterations=8)
        assert np.array_equal(_bits(U8[:, k]), _bits(u)) and its8[k] == it


# ---- moments

@pytest.mark.parametrize("K", [1, 2, 7])
def test_ensemble_moments_equal_numpy_loop(K):
    import slod_amd
    torch, dev = _torch()
    g = slod_amd.Slod(nref=2, n_sub=2, oversampling=1)
    n, ld = 1001, 1004
    rng = np.random.default_rng(100 + K)
    x = rng.standard_normal((K, ld)) * np.exp(rng.uniform(-3.0, 3.0, (1, ld)))
    xt = torch.from_numpy(x).to(dev)
    mean, var = _nan(n + 1), _nan(n + 1)
    torch.cuda.synchronize()
    g.ensemble_moments(xt.data_ptr(), K, n, mean.data_ptr(), var.data_ptr(), ld_fine=ld)
    torch.cuda.synchronize()
    m, v = _moments_numpy(x[:, :n])
    assert np.array_equal(_bits(mean[:n]), m.view(np.uint64))
    assert np.array_equal(_bits(var[:n]), v.view(np.uint64))
    assert torch.isnan(mean[n]) and torch.isnan(var[n])
    if K == 1:
        assert (var[:n] == 0.0).all()
    only = _nan(n)
    g.ensemble_moments(xt.data_ptr(), K, n, only.data_ptr(), None, ld_fine=ld)      # d_var = NULL
    torch.cuda.synchronize()
    assert np.array_equal(_bits(only), m.view(np.uint64))


# ---- end to end

@pytest.mark.parametrize("name", NAMES)
def test_pipeline_moments_equal_three_single_pipelines(so, name):
    torch, dev = _torch()
    c = _case(so, name)
    K = c.K
    V = _nan(c.nval, K)
    cols = torch.zeros_like(c.cols)
    R, U, fine = _nan(c.nrow, K), _nan(c.nrow, K), _nan(K, c.field)
    mean, var = _nan(c.field), _nan(c.field)
    torch.cuda.synchronize()
    c.g.lod_matrix_ensemble(c.b.data_ptr(), c.q.data_ptr(), c.stride, K, V.data_ptr(), cols.data_ptr())
    c.g.lod_rhs_ensemble(c.b.data_ptr(), c.stride, K, c.load.data_ptr(), R.data_ptr())
    its, res = c.g.lod_solve_ensemble(V.data_ptr(), cols.data_ptr(), R.data_ptr(), U.data_ptr(), K, rel_tol=TOL)
    c.g.lod_reconstruct_ensemble(c.b.data_ptr(), c.stride, K, U.data_ptr(), fine.data_ptr())
    c.g.ensemble_moments(fine.data_ptr(), K, c.field, mean.data_ptr(), var.data_ptr())
    torch.cuda.synchronize()
    single = np.stack([_single_reconstruct(c, k, c.sol[k][0]).cpu().numpy() for k in range(K)])
    assert np.array_equal(_bits(fine), single.view(np.uint64))
    m, v = _moments_numpy(single)
    assert np.array_equal(_bits(mean), m.view(np.uint64))
    assert np.array_equal(_bits(var), v.view(np.uint64))
    assert (res <= TOL).all() and v.max() > 0.0
