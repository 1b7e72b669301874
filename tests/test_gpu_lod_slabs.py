"""GPU tests of the slab consumers (slod_lod_matrix, slod_lod_mass_matrix, slod_lod_rhs, slod_lod_reconstruct, their
_multi, _ensemble and _update forms) on slabs that are NOT a basis: every word of every patch vector is random, rims
and domain boundary included, and every word a consumer must not read is NaN (between s n_fine(p) and the stride,
between the members of an ensemble, in the padding of every multi-vector).  A basis vanishes on every patch rim, so
the tests that feed these kernels a basis cannot see an overlap rectangle that is a node short or long, a rim row
taken from the wrong patch, or an x / y or component mix-up; these can.

Geometries (lod_cases.SLAB_CONFIGS): golden, rowmajor, wide (2 l + 1 > N, n_sub 1), mixed (full and clipped patches,
pairs that share a line or nothing), whole (l >= N).  The stride is that of an empty plan; every test runs a second
time with stride + 5.

Bar of every value comparison (lod_cases._slab_bar): |got - ref| <= (m + 16) 2^-53 S_abs, ref and S_abs accumulated in
np.longdouble by lod_cases._ref_*, m the number of terms of the sum.  It is derived, not measured: an index error
moves an entry by O(1) S_abs / sqrt(m).  Everything else is equality of 64-bit words.  The references are checked on
the CPU by test_lod_slab_reference.py.  The worst |got - ref| / bound the tests print are recorded in DESIGN section 6,
"Slab consumers on random slabs".
"""
import numpy as np
import pytest

from lod_cases import (NAN, SLAB_CONFIGS, UNUSED, _Case, _bits, _blocks_by_column, _layout_geometry, _mk, _random_slab, _ref_mass,
                       _ref_matrix, _ref_reconstruct, _ref_rhs, _slab_bar, _slot_columns, _torch)

pytestmark = pytest.mark.gpu

GEOMS = tuple(SLAB_CONFIGS)
PADS = (0, 5)
K = 3                      # ensemble members
SENTINEL = 0x5a5a5a5a      # what the tests write to columns the call must leave alone
_setups, _devs = {}, {}


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _nan(*shape):
    torch, dev = _torch()
    return torch.full(shape, NAN, dtype=torch.float64, device=dev)


def _sentinel(n):
    torch, dev = _torch()
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=dev)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _sync():
    _torch()[0].cuda.synchronize()


def _setup(so, name):
    """Handle, geometry, the stride of an empty plan, host inputs and (lazily) the references; once per geometry."""
    if name not in _setups:
        c = _Case()
        kw = SLAB_CONFIGS[name]
        _, c.g = _mk(so, stabilize=1, **kw)
        c.name, c.geom = name, _layout_geometry(kw, c.g.patch_layout)
        geom = c.geom
        c.s, c.NP, c.cap = geom.s, geom.NP, geom.cap
        c.words = c.NP * c.cap * c.s * c.s
        assert c.g.num_patches == c.NP and c.g.lod_row_capacity() == c.cap
        c.stride0 = c.g.plan(np.zeros(0, dtype=np.uint32)).stride      # returns before a kernel is chosen
        assert c.stride0 >= c.s * geom.n_fine.max()
        rng = np.random.default_rng(1234)
        c.rho = rng.uniform(0.5, 2.0, geom.NE * geom.NE)
        c.f = rng.uniform(-1.0, 1.0, geom.field)                      # non-zero on the domain boundary too
        c.u = rng.uniform(-1.0, 1.0, c.NP * c.s)
        c.Phi, c.Psi = _random_slab(geom, c.stride0, 21)[1][0], _random_slab(geom, c.stride0, 22)[1][0]
        c.refs = {}
        c.all_rows = np.arange(c.NP, dtype=np.uint32)
        _setups[name] = c
    return _setups[name]


def _ref(c, what):
    if what not in c.refs:
        c.refs[what] = {"A": lambda: _ref_matrix(c.geom, c.Phi, c.Psi), "M1": lambda: _ref_mass(c.geom, c.Phi, None),
                        "Mrho": lambda: _ref_mass(c.geom, c.Phi, c.rho), "rhs": lambda: _ref_rhs(c.geom, c.Phi, c.f),
                        "rec": lambda: _ref_reconstruct(c.geom, c.Phi, c.u)}[what]()
    return c.refs[what]


def _device(so, name, pad):
    """The slabs of (phi, psi) with stride = the plan's + pad on the device, and the shared inputs."""
    if (name, pad) not in _devs:
        c = _setup(so, name)
        d = _Case()
        d.stride = c.stride0 + pad
        hb, Phi = _random_slab(c.geom, d.stride, 21)
        hq, Psi = _random_slab(c.geom, d.stride, 22)
        assert all(np.array_equal(a, b) for a, b in zip(Phi[0], c.Phi)) and all(np.array_equal(a, b) for a, b in zip(Psi[0], c.Psi))
        d.b, d.q, d.rho, d.f, d.u = _dev(hb), _dev(hq), _dev(c.rho), _dev(c.f), _dev(c.u)
        _devs[(name, pad)] = d
    return _setup(so, name), _devs[(name, pad)]


# ---- the calls, every output NaN (columns: SENTINEL) beforehand; b, q: device pointers of a slab ----

def _rows(c, kind, b, q, stride, rows, rho=None, extra=0):
    """Block rows of A_LOD ("A") or M_LOD ("M") for `rows`, in arrays with `extra` more rows than the call writes."""
    n = len(rows) + extra
    values, cols = _nan(n * c.cap * c.s * c.s), _sentinel(n * c.cap)
    if kind == "A":
        c.g.lod_matrix(rows, b, q, stride, values.data_ptr(), cols.data_ptr())
    else:
        c.g.lod_mass_matrix(rows, b, stride, values.data_ptr(), cols.data_ptr(), d_rho=rho)
    _sync()
    return values, cols


def _full(c, d, kind):
    """The full call of one kind ("A", "M1": density 1, "Mrho") on the slabs of d, once per (geometry, pad)."""
    if not hasattr(d, "full"):
        d.full = {}
    if kind not in d.full:
        d.full[kind] = _rows(c, kind[0], d.b.data_ptr(), d.q.data_ptr(), d.stride, c.all_rows,
                             rho=d.rho.data_ptr() if kind == "Mrho" else None)
    return d.full[kind]


def _rhs(c, b, stride, rows, f, extra=0):
    out = _nan((len(rows) + extra) * c.s)
    c.g.lod_rhs(rows, b, stride, f, out.data_ptr())
    _sync()
    return out


def _rhs_multi(c, b, stride, rows, F, n_rhs, ld_out, extra=0):
    out = _nan(len(rows) * c.s + extra, ld_out)
    c.g.lod_rhs_multi(rows, b, stride, F.data_ptr(), F.shape[1], n_rhs, out.data_ptr(), ld_out)
    _sync()
    return out


def _reconstruct(c, b, stride, u):
    fine = _nan(c.geom.field)
    c.g.lod_reconstruct(b, stride, u, fine.data_ptr())
    _sync()
    return fine


def _fields(c, n, seed, first=None):
    """n fine fields as rows of a [n][field + 3] array with NaN padding; row 0 is `first` when given."""
    rng = np.random.default_rng(seed)
    h = rng.uniform(-1.0, 1.0, (n, c.geom.field))
    if first is not None:
        h[0] = first
    F = _nan(n, c.geom.field + 3)
    F[:, :c.geom.field] = _dev(h)
    return F


def _check(c, pad, what, got, ref, sabs, m):
    ok, worst = _slab_bar(got, ref, sabs, m)
    print("%s %s stride + %d: worst |got - ref| / bound = %.3f" % (what, c.name, pad, worst))
    assert ok, (what, c.name, pad, worst)


def _used_blocks(c, values, cols, shared):
    """[NP][NP][s][s] of a full call, after the columns were checked against the pattern."""
    assert np.array_equal(_u32(cols).reshape(c.NP, c.cap), _slot_columns(c.geom, shared))
    return _blocks_by_column(c.geom, values.cpu().numpy(), _u32(cols))


# ---- 1. pattern ----

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_pattern_and_unused_slots(so, name, pad):
    """d_cols of both matrices, slot by slot, against "the closed rectangles intersect" written from the extents; the
    same set from slod_lod_pattern; unused slots hold +0."""
    c, d = _device(so, name, pad)
    shared = _ref(c, "A")[3]
    want = _slot_columns(c.geom, shared)
    for kind in ("A", "M1", "Mrho"):
        values, cols = _full(c, d, kind)
        hc = _u32(cols).reshape(c.NP, c.cap)
        assert np.array_equal(hc, want), kind
        words = _bits(values).reshape(c.NP, c.cap, c.s * c.s)
        assert (words[hc == UNUSED] == 0).all(), kind
    for p in range(c.NP):
        assert c.g.lod_pattern(p) == [int(q) for q in np.nonzero(shared[p])[0]]
    if name == "wide":
        assert shared.all()                                   # 2 l + 1 > N: every pair overlaps
    if name == "whole":
        assert shared.all() and (want == UNUSED).sum() == c.NP * (c.cap - c.NP)
    if name == "mixed":
        assert not shared.all()                               # centres further apart than 2 l + 1 share nothing


# ---- 2. A_LOD ----

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_matrix_entries(so, name, pad):
    """Every used entry of A_LOD, all s x s words of a block (the reference is not symmetric in (d, e) nor in
    (phi, psi): orientation and the roles of the two slabs are pinned)."""
    c, d = _device(so, name, pad)
    ref, sabs, m, shared = _ref(c, "A")
    values, cols = _full(c, d, "A")
    got = _used_blocks(c, values, cols, shared)
    assert np.isfinite(values.cpu().numpy()).all()
    _check(c, pad, "A_LOD", got, ref, sabs, m[:, :, None, None])


# ---- 3. M_LOD ----

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_mass_entries_symmetry_and_line_pairs(so, name, pad):
    c, d = _device(so, name, pad)
    lines = 0
    for kind in ("M1", "Mrho"):
        ref, sabs, m, shared = _ref(c, kind)
        values, cols = _full(c, d, kind)
        got = _used_blocks(c, values, cols, shared)
        assert np.isfinite(values.cpu().numpy()).all()
        _check(c, pad, "M_LOD (%s)" % ("rho = 1" if kind == "M1" else "random rho"), got, ref, sabs, m[:, :, None, None])
        # pairs that share only a line of nodes: in the pattern (checked by _used_blocks), value +0
        line = shared & (m == 0)
        lines = int(line.sum())
        assert (got.view(np.uint64)[line] == 0).all()
        # M[(p,d),(q,e)] and M[(q,e),(p,d)] are the same words
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(got.transpose(1, 0, 3, 2)).view(np.uint64))
    if name in ("mixed", "rowmajor", "golden"):
        assert lines > 0                                      # the geometry has such pairs


# ---- 4. C^T f ----

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_rhs_and_rhs_multi(so, name, pad):
    c, d = _device(so, name, pad)
    ref, sabs, m = _ref(c, "rhs")
    one = _rhs(c, d.b.data_ptr(), d.stride, c.all_rows, d.f.data_ptr())
    _check(c, pad, "C^T f", one.cpu().numpy(), ref, sabs, m)
    for n_rhs in (3, 65):
        F = _fields(c, n_rhs, 31, first=c.f)
        ld_out = n_rhs + 2
        out = _rhs_multi(c, d.b.data_ptr(), d.stride, c.all_rows, F, n_rhs, ld_out)
        assert np.array_equal(_bits(out[:, 0]), _bits(one))
        for k in range(1, n_rhs):
            col = _rhs(c, d.b.data_ptr(), d.stride, c.all_rows, F[k].data_ptr())
            assert np.array_equal(_bits(out[:, k]), _bits(col)), (n_rhs, k)
        assert bool(_torch()[0].isnan(out[:, n_rhs:]).all())


# ---- 5. C u ----

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_reconstruct_and_reconstruct_multi(so, name, pad):
    torch, dev = _torch()
    c, d = _device(so, name, pad)
    ref, sabs, m = _ref(c, "rec")
    one = _reconstruct(c, d.b.data_ptr(), d.stride, d.u.data_ptr())
    _check(c, pad, "C u", one.cpu().numpy().reshape(ref.shape), ref, sabs, m)     # every fine node, domain corners included
    n_rhs, ld_u = 3, 5
    hu = np.random.default_rng(41).uniform(-1.0, 1.0, (c.NP * c.s, n_rhs))
    hu[:, 0] = c.u
    U = _nan(c.NP * c.s, ld_u)
    U[:, :n_rhs] = _dev(hu)
    fine = _nan(n_rhs + 1, c.geom.field + 3)
    c.g.lod_reconstruct_multi(d.b.data_ptr(), d.stride, U.data_ptr(), ld_u, n_rhs, fine.data_ptr(), fine.shape[1])
    _sync()
    assert np.array_equal(_bits(fine[0, :c.geom.field]), _bits(one))
    for k in range(1, n_rhs):
        uk = _dev(hu[:, k])
        col = _reconstruct(c, d.b.data_ptr(), d.stride, uk.data_ptr())
        assert np.array_equal(_bits(fine[k, :c.geom.field]), _bits(col)), k
    assert bool(torch.isnan(fine[:, c.geom.field:]).all()) and bool(torch.isnan(fine[n_rhs]).all())
    assert bool(torch.isnan(U[:, n_rhs:]).all())


# ---- 6. row subsets ----

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_row_subsets(so, name, pad):
    """rows = a seeded permutation of about half the patches with one id repeated (what a rank of a distributed run
    passes): output row k has the words of row rows[k] of the full call, and nothing from row n_rows on is written."""
    torch, dev = _torch()
    c, d = _device(so, name, pad)
    s, cap = c.s, c.cap
    rows = np.random.default_rng(51).permutation(c.NP)[:c.NP // 2 + 1].astype(np.uint32)
    rows = np.concatenate([rows, rows[1:2]])
    n = len(rows)
    assert not np.array_equal(rows, np.sort(rows)) and len(set(rows.tolist())) == n - 1
    idx = rows.astype(np.int64)
    for kind in ("A", "M1", "Mrho"):
        fv, fc = _full(c, d, kind)
        values, cols = _rows(c, kind[0], d.b.data_ptr(), d.q.data_ptr(), d.stride, rows,
                             rho=d.rho.data_ptr() if kind == "Mrho" else None, extra=2)
        assert np.array_equal(_bits(values).reshape(n + 2, -1)[:n], _bits(fv).reshape(c.NP, -1)[idx]), kind
        assert np.array_equal(_u32(cols).reshape(n + 2, cap)[:n], _u32(fc).reshape(c.NP, cap)[idx]), kind
        assert bool(torch.isnan(values[n * cap * s * s:]).all()) and (_u32(cols)[n * cap:] == SENTINEL).all(), kind
    full = _rhs(c, d.b.data_ptr(), d.stride, c.all_rows, d.f.data_ptr())
    sub = _rhs(c, d.b.data_ptr(), d.stride, rows, d.f.data_ptr(), extra=2)
    assert np.array_equal(_bits(sub).reshape(n + 2, s)[:n], _bits(full).reshape(c.NP, s)[idx])
    assert bool(torch.isnan(sub[n * s:]).all())
    F = _fields(c, 3, 52, first=c.f)
    mfull = _rhs_multi(c, d.b.data_ptr(), d.stride, c.all_rows, F, 3, 4)
    msub = _rhs_multi(c, d.b.data_ptr(), d.stride, rows, F, 3, 4, extra=2 * s)
    assert np.array_equal(_bits(mfull[:, 0]), _bits(full))
    assert np.array_equal(_bits(msub[:n * s, :3]).reshape(n, s, 3), _bits(mfull[:, :3]).reshape(c.NP, s, 3)[idx])
    assert bool(torch.isnan(msub[n * s:]).all()) and bool(torch.isnan(msub[:, 3:]).all())


# ---- 7. ensemble forms ----

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_ensemble_members_equal_single_calls(so, name, pad):
    """K = 3 members, member_stride = num_patches stride + 7 with NaN in the gap, ld_m = K + 2, ld_out = K + 1: member k
    has the words of the single call on its slab, the padding columns stay NaN, and a member sub-range (base + first
    member) gives the same words."""
    torch, dev = _torch()
    c, d = _device(so, name, pad)
    s, cap, NP, geom = c.s, c.cap, c.NP, c.geom
    stride, mstride, ld_m, ld_out = d.stride, NP * d.stride + 7, K + 2, K + 1
    B, Q = _dev(_random_slab(geom, stride, 61, members=K, member_gap=7)[0]), _dev(_random_slab(geom, stride, 62, members=K, member_gap=7)[0])
    bp = [B.data_ptr() + 8 * k * mstride for k in range(K)]
    qp = [Q.data_ptr() + 8 * k * mstride for k in range(K)]
    rho_ld = geom.NE * geom.NE + 1
    RHO = _nan(K, rho_ld)
    RHO[:, :rho_ld - 1] = _dev(np.random.default_rng(63).uniform(0.5, 2.0, (K, rho_ld - 1)))
    F = _fields(c, K, 64)
    hu = np.random.default_rng(65).uniform(-1.0, 1.0, (NP * s, K))
    U = _nan(NP * s, ld_out)
    U[:, :K] = _dev(hu)

    def matrix_like(call, single):
        """call(b0, first, n, values_ptr, cols_ptr) runs members first .. first + n; single(k) -> (values, cols)."""
        values, cols = _nan(c.words, ld_m), _sentinel(NP * cap)
        call(0, K, values.data_ptr(), cols.data_ptr())
        part, pcols = _nan(c.words, ld_m), _sentinel(NP * cap)
        call(1, K - 1, part.data_ptr() + 8, pcols.data_ptr())
        _sync()
        for k in range(K):
            sv, sc = single(k)
            assert np.array_equal(_bits(values[:, k]), _bits(sv)), k
            assert np.array_equal(_u32(cols), _u32(sc)) and np.array_equal(_u32(pcols), _u32(sc))
        assert bool(torch.isnan(values[:, K:]).all())
        assert np.array_equal(_bits(part[:, 1:K]), _bits(values[:, 1:K]))
        assert bool(torch.isnan(part[:, 0]).all()) and bool(torch.isnan(part[:, K:]).all())

    matrix_like(lambda first, n, v, cl: c.g.lod_matrix_ensemble(bp[first], qp[first], stride, n, v, cl, member_stride=mstride, ld_m=ld_m),
                lambda k: _rows(c, "A", bp[k], qp[k], stride, c.all_rows))
    matrix_like(lambda first, n, v, cl: c.g.lod_mass_matrix_ensemble(bp[first], stride, n, v, cl, d_rho=d.rho.data_ptr(), ld_rho=0,
                                                                     member_stride=mstride, ld_m=ld_m),
                lambda k: _rows(c, "M", bp[k], None, stride, c.all_rows, rho=d.rho.data_ptr()))
    matrix_like(lambda first, n, v, cl: c.g.lod_mass_matrix_ensemble(bp[first], stride, n, v, cl, d_rho=RHO[first].data_ptr(), ld_rho=rho_ld,
                                                                     member_stride=mstride, ld_m=ld_m),
                lambda k: _rows(c, "M", bp[k], None, stride, c.all_rows, rho=RHO[k].data_ptr()))

    # C^T f: one load for all members (ld_fine = 0), then a load per member
    for ld_fine in (0, F.shape[1]):
        out, part = _nan(NP * s, ld_out), _nan(NP * s, ld_out)
        c.g.lod_rhs_ensemble(bp[0], stride, K, F.data_ptr(), out.data_ptr(), ld_fine=ld_fine, member_stride=mstride, ld_out=ld_out)
        c.g.lod_rhs_ensemble(bp[1], stride, K - 1, F[1 if ld_fine else 0].data_ptr(), part.data_ptr() + 8, ld_fine=ld_fine,
                             member_stride=mstride, ld_out=ld_out)
        _sync()
        for k in range(K):
            one = _rhs(c, bp[k], stride, c.all_rows, F[k if ld_fine else 0].data_ptr())
            assert np.array_equal(_bits(out[:, k]), _bits(one)), (ld_fine, k)
        assert bool(torch.isnan(out[:, K:]).all())
        assert np.array_equal(_bits(part[:, 1:K]), _bits(out[:, 1:K])) and bool(torch.isnan(part[:, 0]).all()) and bool(torch.isnan(part[:, K:]).all())

    # C u
    ld_fine = geom.field + 3
    fine, part = _nan(K, ld_fine), _nan(K, ld_fine)
    c.g.lod_reconstruct_ensemble(bp[0], stride, K, U.data_ptr(), fine.data_ptr(), ld_fine=ld_fine, member_stride=mstride, ld_u=ld_out)
    c.g.lod_reconstruct_ensemble(bp[1], stride, K - 1, U.data_ptr() + 8, part[1].data_ptr(), ld_fine=ld_fine, member_stride=mstride,
                                 ld_u=ld_out)
    _sync()
    for k in range(K):
        uk = _dev(hu[:, k])
        one = _reconstruct(c, bp[k], stride, uk.data_ptr())
        assert np.array_equal(_bits(fine[k, :geom.field]), _bits(one)), k
    assert bool(torch.isnan(fine[:, geom.field:]).all())
    assert np.array_equal(_bits(part[1:, :geom.field]), _bits(fine[1:, :geom.field]))
    assert bool(torch.isnan(part[0]).all()) and bool(torch.isnan(part[:, geom.field:]).all())


# ---- 8. in-place update ----

def _dirty_sets(c):
    """{a corner patch}; {an interior patch, a rim patch}; the empty set; all patches -- by centre cell."""
    pid = c.geom.pid
    return [("corner", [pid[(0, 0)]]), ("interior + rim", [pid[(1, 1)], pid[(1, 0)]]), ("none", []), ("all", list(range(c.NP)))]


def _flags(c, patches):
    torch, dev = _torch()
    h = np.zeros(c.NP, dtype=np.int32)
    h[patches] = 1
    return torch.from_numpy(h).to(dev), h.astype(bool)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_update_rewrites_dirty_entries_and_nothing_else(so, name, pad):
    """Block rows built from slabs S0, then slod_lod_matrix_update / slod_lod_mass_matrix_update on slabs S1 that
    differ from S0 in every patch: a used entry with a dirty row or column has the words of the full call on S1, every
    other word of d_values those from S0 -- which, S1 differing everywhere, proves nothing else was written."""
    torch, dev = _torch()
    c, d = _device(so, name, pad)
    geom, stride = c.geom, d.stride
    h1b, P1 = _random_slab(geom, stride, 71)
    h1q, Q1 = _random_slab(geom, stride, 72)
    assert all(not np.array_equal(a, b) for a, b in zip(P1[0], c.Phi)) and all(not np.array_equal(a, b) for a, b in zip(Q1[0], c.Psi))
    b1, q1 = _dev(h1b), _dev(h1q)
    assert geom.N >= 3                                        # a corner, a rim and an interior centre exist
    for kind in ("A", "Mrho"):
        v0, cols = _full(c, d, kind)
        v1, cols1 = _rows(c, kind[0], b1.data_ptr(), q1.data_ptr(), stride, c.all_rows, rho=d.rho.data_ptr())
        hc = _u32(cols).reshape(c.NP, c.cap)
        assert np.array_equal(hc, _u32(cols1).reshape(c.NP, c.cap))
        w0, w1 = _bits(v0).reshape(c.NP, c.cap, -1), _bits(v1).reshape(c.NP, c.cap, -1)
        used = hc != UNUSED
        # the full calls differ in every used word (of the mass: of the pairs that share an element)
        differ = used if kind == "A" else used & (_ref(c, kind)[2][np.arange(c.NP)[:, None], np.where(used, hc, 0).astype(np.int64)] > 0)
        assert differ.any() and (w0[differ] != w1[differ]).all()
        for label, patches in _dirty_sets(c):
            flags, dirty = _flags(c, patches)
            vals = v0.clone()
            if kind == "A":
                c.g.lod_matrix_update(flags.data_ptr(), b1.data_ptr(), q1.data_ptr(), stride, vals.data_ptr())
            else:
                c.g.lod_mass_matrix_update(flags.data_ptr(), b1.data_ptr(), stride, vals.data_ptr(), d_rho=d.rho.data_ptr())
            _sync()
            touched = used & (dirty[:, None] | dirty[np.where(used, hc, 0).astype(np.int64)])
            want = np.where(touched[:, :, None], w1, w0)
            assert np.array_equal(_bits(vals).reshape(want.shape), want), (kind, label)
            assert (not touched.any()) if label == "none" else np.array_equal(touched, used) if label == "all" else touched.any()
            assert np.array_equal(flags.cpu().numpy().astype(bool), dirty)          # the flags are read only
    # member 1 of a K = 3 ensemble matrix: d_values + 1, ld_m = 3
    mstride = c.NP * stride + 7
    E0b, E0q = _dev(_random_slab(geom, stride, 73, members=K, member_gap=7)[0]), _dev(_random_slab(geom, stride, 74, members=K, member_gap=7)[0])
    ens, ecols = _nan(c.words, K), _sentinel(c.NP * c.cap)
    c.g.lod_matrix_ensemble(E0b.data_ptr(), E0q.data_ptr(), stride, K, ens.data_ptr(), ecols.data_ptr(), member_stride=mstride, ld_m=K)
    _sync()
    before = _bits(ens).copy()
    hc = _u32(ecols).reshape(c.NP, c.cap)
    used = hc != UNUSED
    flags, dirty = _flags(c, _dirty_sets(c)[1][1])
    c.g.lod_matrix_update(flags.data_ptr(), b1.data_ptr(), q1.data_ptr(), stride, ens.data_ptr() + 8, ld_m=K)
    _sync()
    v1, _ = _rows(c, "A", b1.data_ptr(), q1.data_ptr(), stride, c.all_rows)
    touched = used & (dirty[:, None] | dirty[np.where(used, hc, 0).astype(np.int64)])
    want = before.reshape(c.NP, c.cap, -1, K).copy()
    want[:, :, :, 1] = np.where(touched[:, :, None], _bits(v1).reshape(c.NP, c.cap, -1), want[:, :, :, 1])
    assert np.array_equal(_bits(ens).reshape(want.shape), want)
    assert 0 < touched.sum() < used.sum() or name in ("wide", "whole")   # there every row couples with every patch
