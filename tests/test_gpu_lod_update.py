"""The refresh after a local coefficient change on the GPU: slod_update_coefficient flags exactly the patches whose extent
holds a changed fine element, the dirty plan rebuilds exactly those in place, and the matrix updates recompute exactly
the entries with a dirty row or column, each with the bits of a full rebuild on the refreshed slabs.

One scenario per configuration, built once and only read by the tests: the old build in NaN-padded slabs, the change of
the table below, the refreshed slabs, and a full rebuild on the changed coefficient."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import make_fields
from lod_cases import MASS_CONFIGS, NAN, PENCIL_CONFIGS, TOL_PHI, _bits, _check_patch, _lod_matrix, _rows_to_dense, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
# name -> (configuration, [(field, ex, ey)] changed elements, number of dirty patches)
#   step64   N = 8, l = 1, n = 2: one element of cell (3, 3); the 9 dirty patches are full interior patches
#   s1       N = 4, l = 1: element (0, 0)
#   clipped  N = 4, l = 2, n = 4: one element of cell (0, 0); 9 of 16, and no patch of this grid is full
#   rowmajor N = 5, n = 3, l = 1: the last element of the domain
#   s2       elasticity: only mu in cell (0, 0), then only lambda in cell (3, 3): the union, 4 + 4
CASES = {"step64": (PENCIL_CONFIGS["step64"], [(0, 7, 6)], 9),
         "s1": (MASS_CONFIGS["s1"], [(0, 0, 0)], 4),
         "clipped": (MASS_CONFIGS["clipped"], [(0, 2, 1)], 9),
         "rowmajor": (MASS_CONFIGS["rowmajor"], [(0, 14, 14)], 4),
         "s2": (MASS_CONFIGS["s2"], [(1, 1, 0), (0, 6, 7)], 8)}
NAMES = sorted(CASES)
SENTINEL = np.uint64(0x7ff8dead0000beef)     # a NaN with a payload no kernel produces
_cache = {}


class _Scenario:
    pass


def _handle(so, kw, n_problems=1):
    import slod_amd
    cfg = so.make_cfg(stabilize=1, **kw)
    g = slod_amd.Slod(nref=kw.get("nref", 0), n_sub=kw["n_sub"], oversampling=kw["oversampling"],
                      spacedim=kw.get("spacedim", 1), n_cells=kw.get("n_cells", 0), n_problems=n_problems)
    return cfg, g


def _nan(*shape):
    torch, dev = _torch()
    return torch.full(shape, NAN, dtype=torch.float64, device=dev)


def _zero_dirty(g):
    torch, dev = _torch()
    return torch.zeros(g.num_patches, dtype=torch.int32, device=dev)


def _flags(d):
    return d.cpu().numpy().view(np.uint32)


def _rule(g, changed):
    """the patches whose extent holds a changed fine element; changed: bool [NE][NE] (ey, ex)"""
    n = g.cfg.n_subdivisions
    out = []
    for p in range(g.num_patches):
        i = g.patch_layout(p)
        if changed[i.y0 * n:(i.y0 + i.my) * n, i.x0 * n:(i.x0 + i.mx) * n].any():
            out.append(p)
    return np.array(out, dtype=np.int64)


def _changed(old, new, NE):
    """elements with a changed stored word; old, new: layout 1 arrays"""
    return (old.view(np.uint64) != new.view(np.uint64)).reshape(NE, NE, 4).any(axis=2)


def _execute(plan, b, q):
    torch, dev = _torch()
    torch.cuda.synchronize()
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    torch.cuda.synchronize()


def _full_build(g, problem=0):
    """every patch of one problem into NaN-filled uniform-stride slabs"""
    NP = g.num_patches
    plan = g.plan(np.arange(problem * NP, (problem + 1) * NP, dtype=np.uint32))
    b, q = _nan(NP * plan.stride), _nan(NP * plan.stride)
    _execute(plan, b, q)
    return b, q, plan.stride


def _assert_stored(so, g, kw, fields, problem=0):
    """the stored field is what slod_set_coefficient stores: a plan on it gives the bits of a fresh handle's"""
    _, fresh = _handle(so, kw)
    for f, a in enumerate(fields):
        fresh.set_coefficient(f, a)
    b, q, _ = _full_build(g, problem)
    fb, fq, _ = _full_build(fresh)
    assert np.array_equal(_bits(b), _bits(fb)) and np.array_equal(_bits(q), _bits(fq))


def _scale(fields, field, ex, ey, NE, factor=1.5):
    out = [a.copy() for a in fields]
    out[field][(ey * NE + ex) * 4:(ey * NE + ex) * 4 + 4] *= factor
    return out


def _scenario(so, name):
    if name in _cache:
        return _cache[name]
    torch, dev = _torch()
    kw, changes, count = CASES[name]
    c = _Scenario()
    c.kw, c.s, c.count = kw, kw.get("spacedim", 1), count
    c.cfg, g = _handle(so, kw)
    c.g, NE, NP = g, g.NE, g.num_patches
    c.old = make_fields(so, c.cfg, "D100")
    for f, a in enumerate(c.old):
        g.set_coefficient(f, a)
    c.b0, c.q0, c.stride = _full_build(g)
    c.A0, c.cols = _lod_matrix(g, c.b0, c.q0, c.stride, c.s)
    # the change: one call per changed field on one dirty array
    c.new = c.old
    c.dirty = _zero_dirty(g)
    for field, ex, ey in changes:
        c.new = _scale(c.new, field, ex, ey, NE)
        g.update_coefficient(field, c.new[field], c.dirty.data_ptr())
    c.ids = g.dirty_patches(c.dirty.data_ptr())
    changed = np.zeros((NE, NE), dtype=bool)
    for f in range(c.s):
        changed |= _changed(c.old[f], c.new[f], NE)
    c.expect = _rule(g, changed)
    # refresh in place on copies of the old slabs
    c.plan = g.plan_dirty(c.dirty.data_ptr())
    c.b1, c.q1 = c.b0.clone(), c.q0.clone()
    _execute(c.plan, c.b1, c.q1)
    c.A1 = c.A0.clone()
    torch.cuda.synchronize()
    g.lod_matrix_update(c.dirty.data_ptr(), c.b1.data_ptr(), c.q1.data_ptr(), c.stride, c.A1.data_ptr())
    torch.cuda.synchronize()
    # the references: A_LOD on the refreshed slabs, and a full rebuild with the changed coefficient
    c.Aref, cols = _lod_matrix(g, c.b1, c.q1, c.stride, c.s)
    assert torch.equal(cols, c.cols)
    c.bf, c.qf, _ = _full_build(g)
    c.hcols = c.cols.cpu().numpy().view(np.uint32).reshape(NP, -1)
    f = _flags(c.dirty) != 0
    used = c.hcols != 0xffffffff
    c.mask = used & (f[:, None] | f[np.where(used, c.hcols, 0)])          # [NP][cap]: entries to recompute
    _cache[name] = c
    return c


def _entry_mask(c):
    return np.repeat(c.mask.ravel(), c.s * c.s)


# ---- 1. the dirty set

@pytest.mark.parametrize("name", NAMES)
def test_dirty_set_of_every_configuration(so, name):
    c = _scenario(so, name)
    print("%s: %d of %d patches dirty" % (name, len(c.ids), c.g.num_patches))
    assert np.array_equal(c.ids, c.expect)
    assert len(c.ids) == c.count and c.g.dirty_patches(c.dirty.data_ptr(), count_only=True) == c.count
    assert set(np.unique(_flags(c.dirty)).tolist()) <= {0, 1}
    full = 2 * c.kw["oversampling"] + 1
    sizes = {(c.g.patch_layout(int(p)).mx, c.g.patch_layout(int(p)).my) for p in c.ids}
    if name == "step64":
        assert sizes == {(full, full)}
    if name == "clipped":
        assert all((c.g.patch_layout(p).mx, c.g.patch_layout(p).my) != (full, full) for p in range(c.g.num_patches))
    # a buffer below the count is refused, the array is left alone
    import ctypes as C
    buf = (C.c_uint32 * c.count)()
    assert c.g.lib.slod_dirty_patches(c.g.h, c.dirty.data_ptr(), buf, c.count - 1) == -1
    assert "slod_dirty_patches" in c.g.lib.slod_last_error(c.g.h).decode()
    _assert_stored(so, c.g, c.kw, c.new)


def _fresh(so, kw, per_qp=True):
    """a handle with the D100 field stored (layout 0: the value of slot 0 of every element)"""
    cfg, g = _handle(so, kw)
    fields = make_fields(so, cfg, "D100")
    if not per_qp:
        fields = [np.ascontiguousarray(a.reshape(-1, 4)[:, 0]) for a in fields]
    for f, a in enumerate(fields):
        g.set_coefficient(f, a, per_qp=per_qp)
    return g, fields


def test_dirty_set_of_single_slot_ulp_same_all_and_accumulation(so):
    torch, dev = _torch()
    kw = PENCIL_CONFIGS["step64"]
    g, old = _fresh(so, kw)
    NE, NP = g.NE, g.num_patches
    # the same data again: nothing is dirty, the array stays zero
    d = _zero_dirty(g)
    g.update_coefficient(0, old[0], d.data_ptr())
    assert g.dirty_patches(d.data_ptr(), count_only=True) == 0 and len(g.dirty_patches(d.data_ptr())) == 0
    assert not _flags(d).any()
    # layout 1, only slot q = 3 of element (9, 4) changed, by one ulp
    new = [old[0].copy()]
    at = (4 * NE + 9) * 4 + 3
    new[0][at] = np.nextafter(new[0][at], np.inf)
    g.update_coefficient(0, new[0], d.data_ptr())
    first = g.dirty_patches(d.data_ptr())
    assert np.array_equal(first, _rule(g, _changed(old[0], new[0], NE))) and len(first) == 9
    _assert_stored(so, g, kw, new)
    # flags accumulate over calls; words set by hand survive, also on a patch that becomes dirty
    newer = [new[0].copy()]
    newer[0][(15 * NE + 0) * 4:(15 * NE + 0) * 4 + 4] = 3.25            # element (0, 15): cell (0, 7)
    second = _rule(g, _changed(new[0], newer[0], NE))
    assert len(second) == 4 and not set(second) & set(first)
    clean = int(np.setdiff1d(np.arange(NP), np.concatenate([first, second]))[0])
    hand = _flags(d).copy()
    hand[clean], hand[second[0]] = 6, 4
    d.copy_(torch.from_numpy(hand.view(np.int32)))
    torch.cuda.synchronize()
    g.update_coefficient(0, newer[0], d.data_ptr())
    expect = np.zeros(NP, dtype=np.uint32)
    expect[first], expect[second], expect[clean], expect[second[0]] = 1, 1, 6, 5
    assert np.array_equal(_flags(d), expect)
    assert np.array_equal(g.dirty_patches(d.data_ptr()), np.nonzero(expect)[0])
    _assert_stored(so, g, kw, newer)
    # every element changed: every patch is dirty
    d.zero_()
    g.update_coefficient(0, newer[0] * 2.0, d.data_ptr())
    assert np.array_equal(g.dirty_patches(d.data_ptr()), np.arange(NP))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_dirty_set_layout_0(so, on_device):
    """layout 0: data[i] against the four stored slots of element i"""
    torch, dev = _torch()
    kw = MASS_CONFIGS["rowmajor"]
    g, old = _fresh(so, kw, per_qp=False)
    NE = g.NE
    new = old[0].copy()
    new[7 * NE + 4] *= 1.25                                              # element (4, 7): cell (1, 2)
    new[0] = np.nextafter(new[0], 0.0)
    d = _zero_dirty(g)
    if on_device:
        t = torch.from_numpy(new).to(dev)
        torch.cuda.synchronize()
        g.update_coefficient_device(0, t.data_ptr(), t.numel(), d.data_ptr(), per_qp=False)
    else:
        g.update_coefficient(0, new, d.data_ptr(), per_qp=False)
    changed = (old[0].view(np.uint64) != new.view(np.uint64)).reshape(NE, NE)
    assert changed.sum() == 2
    assert np.array_equal(g.dirty_patches(d.data_ptr()), _rule(g, changed))
    _assert_stored(so, g, kw, [np.repeat(new, 4)])
    # a field stored per quadrature point, updated per element: every element whose four values were not that one changes
    g2, old2 = _fresh(so, kw)
    const_el = (old2[0].reshape(-1, 4) == old2[0].reshape(-1, 4)[:, :1]).all(axis=1)
    per_el = np.ascontiguousarray(old2[0].reshape(-1, 4)[:, 0])
    d2 = _zero_dirty(g2)
    g2.update_coefficient(0, per_el, d2.data_ptr(), per_qp=False)
    assert np.array_equal(g2.dirty_patches(d2.data_ptr()), _rule(g2, ~const_el.reshape(NE, NE)))
    _assert_stored(so, g2, kw, [np.repeat(per_el, 4)])


def test_dirty_set_n_sub_1(so):
    torch, dev = _torch()
    kw = dict(nref=3, n_sub=1, oversampling=1, spacedim=1)
    g, old = _fresh(so, kw)
    new = _scale(old, 0, 5, 2, g.NE)
    d = _zero_dirty(g)
    g.update_coefficient(0, new[0], d.data_ptr())
    ids = g.dirty_patches(d.data_ptr())
    assert np.array_equal(ids, _rule(g, _changed(old[0], new[0], g.NE))) and len(ids) == 9
    # (no patch solve with one fine element per cell: the stored field is read back directly, which
    # slod_coarse_coefficient does for n_subdivisions = 1)
    stored = _nan(g.NE * g.NE * 4)
    g.coarse_coefficient(0, stored.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(stored), new[0].view(np.uint64))


def test_dirty_set_of_one_ensemble_member(so):
    """n_problems = 3: updating problem 1 flags its patches and leaves the stored fields of problems 0 and 2 alone"""
    kw = MASS_CONFIGS["s1"]
    cfg, g = _handle(so, kw, n_problems=3)
    fields = [make_fields(so, cfg, dist) for dist in ("const", "D100", "D1e4")]
    for k, fl in enumerate(fields):
        g.set_coefficient(0, fl[0], problem=k)
    before = [_full_build(g, k) for k in range(3)]
    new = _scale(fields[1], 0, 5, 5, g.NE)
    d = _zero_dirty(g)
    g.update_coefficient(0, new[0], d.data_ptr(), problem=1)
    assert np.array_equal(g.dirty_patches(d.data_ptr()), _rule(g, _changed(fields[1][0], new[0], g.NE)))
    for k in (0, 2):
        b, q, _ = _full_build(g, k)
        assert np.array_equal(_bits(b), _bits(before[k][0])) and np.array_equal(_bits(q), _bits(before[k][1]))
    _assert_stored(so, g, kw, new, problem=1)
    b, _, _ = _full_build(g, 1)
    assert not np.array_equal(_bits(b), _bits(before[1][0]))


# ---- 2. the basis refresh

@pytest.mark.parametrize("name", NAMES)
def test_dirty_plan_rebuilds_the_dirty_patches_in_place(so, name):
    torch, dev = _torch()
    c = _scenario(so, name)
    g, stride, NP = c.g, c.stride, c.g.num_patches
    assert c.plan.stride == stride and len(c.plan.gids) == c.count
    b0, q0, b1, q1 = (_bits(t).reshape(NP, stride) for t in (c.b0, c.q0, c.b1, c.q1))
    hb, hq = c.b1.cpu().numpy(), c.q1.cpu().numpy()
    # the plan slod_plan_create gives for the same list and offsets
    plan = g.plan(c.ids.astype(np.uint32), c.ids.astype(np.uint64) * np.uint64(stride))
    b2, q2 = c.b0.clone(), c.q0.clone()
    _execute(plan, b2, q2)
    assert np.array_equal(_bits(b2), b1.ravel()) and np.array_equal(_bits(q2), q1.ravel())
    dirty = set(c.ids.tolist())
    worst = 0.0
    for p in range(NP):
        size = c.s * g.patch_layout(p).n_fine
        assert np.isnan(hb[p * stride + size:(p + 1) * stride]).all() and np.isnan(hq[p * stride + size:(p + 1) * stride]).all()
        if p in dirty:
            assert not np.array_equal(b1[p, :size], b0[p, :size]), (name, p)
            worst = max(worst, *_check_patch(so, c.cfg, c.new, p, hb, hq, p * stride, label=name))
        else:   # the old words, the gap up to the stride included
            assert np.array_equal(b1[p], b0[p]) and np.array_equal(q1[p], q0[p]), (name, p)
    print("%s: worst deviation of a refreshed patch from the oracle %.3e" % (name, worst))
    same = np.array_equal(b1.ravel(), _bits(c.bf)) and np.array_equal(q1.ravel(), _bits(c.qf))
    print("%s: refreshed slab bit-equal to a full rebuild: %s" % (name, same))
    if name == "step64":        # full interior patches in the list: the maxima, hence the kernel, of the full plan
        assert same
    else:                       # no bit contract here, but the refreshed slab is a full rebuild to the basis accuracy
        fb = c.bf.cpu().numpy()
        ok = ~np.isnan(fb)
        assert np.abs(hb[ok] - fb[ok]).max() <= 2 * TOL_PHI


def test_empty_dirty_plan_writes_nothing(so):
    c = _scenario(so, "s1")
    d = _zero_dirty(c.g)
    plan = c.g.plan_dirty(d.data_ptr())
    assert len(plan.gids) == 0 and plan.stride == c.stride
    b, q = _nan(c.g.num_patches * c.stride), _nan(c.g.num_patches * c.stride)
    _execute(plan, b, q)
    torch, dev = _torch()
    assert torch.isnan(b).all() and torch.isnan(q).all()


# ---- 3. the matrix update

def _sentinel_like(t):
    torch, dev = _torch()
    return torch.from_numpy(np.full(t.numel(), SENTINEL, dtype=np.uint64).view(np.float64)).to(dev)


def _assert_exactly_the_dirty_entries(c, got, fresh, label):
    got, fresh = _bits(got), _bits(fresh)
    m = _entry_mask(c)
    assert m.any() and not m.all()
    assert np.array_equal(got[m], fresh[m]), label
    assert (got[~m] == SENTINEL).all(), label


@pytest.mark.parametrize("name", NAMES)
def test_matrix_update_equals_fresh_matrix(so, name):
    torch, dev = _torch()
    c = _scenario(so, name)
    g = c.g
    assert np.array_equal(_bits(c.A1), _bits(c.Aref)), name
    assert not np.array_equal(_bits(c.A0), _bits(c.Aref))
    print("%s: %d of %d used entries recomputed" % (name, c.mask.sum(), (c.hcols != 0xffffffff).sum()))
    # on a sentinel-filled array: exactly the entries with a dirty row or column are written
    S = _sentinel_like(c.A0)
    torch.cuda.synchronize()
    g.lod_matrix_update(c.dirty.data_ptr(), c.b1.data_ptr(), c.q1.data_ptr(), c.stride, S.data_ptr())
    torch.cuda.synchronize()
    _assert_exactly_the_dirty_entries(c, S, c.Aref, name)
    # no patch dirty: nothing is written
    none = _zero_dirty(g)
    S = _sentinel_like(c.A0)
    torch.cuda.synchronize()
    g.lod_matrix_update(none.data_ptr(), c.b1.data_ptr(), c.q1.data_ptr(), c.stride, S.data_ptr())
    torch.cuda.synchronize()
    assert (_bits(S) == SENTINEL).all()
    # every patch dirty (any non-zero word): the full matrix
    every = torch.full_like(none, 2)
    A = c.A0.clone()
    torch.cuda.synchronize()
    g.lod_matrix_update(every.data_ptr(), c.b1.data_ptr(), c.q1.data_ptr(), c.stride, A.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(A), _bits(c.Aref))


def test_matrix_update_of_one_ensemble_member(so):
    """K = 3 on a padded ld_m = 5, member 1 refreshed: its words equal a fresh slod_lod_matrix_ensemble, the members
    0 and 2 and the padding are untouched"""
    torch, dev = _torch()
    kw = MASS_CONFIGS["s1"]
    cfg, g = _handle(so, kw, n_problems=3)
    fields = [make_fields(so, cfg, dist) for dist in ("const", "D100", "D1e4")]
    for k, fl in enumerate(fields):
        g.set_coefficient(0, fl[0], problem=k)
    K, ld, NP, cap = 3, 5, g.num_patches, g.lod_row_capacity()
    plan = g.plan(np.arange(K * NP, dtype=np.uint32))
    stride, mstride = plan.stride, NP * plan.stride
    b, q = _nan(K * mstride), _nan(K * mstride)
    _execute(plan, b, q)
    V = _nan(NP * cap, ld)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    g.lod_matrix_ensemble(b.data_ptr(), q.data_ptr(), stride, K, V.data_ptr(), cols.data_ptr(), ld_m=ld)
    torch.cuda.synchronize()
    old = V.clone()
    new = _scale(fields[1], 0, 2, 3, g.NE)
    d = _zero_dirty(g)
    g.update_coefficient(0, new[0], d.data_ptr(), problem=1)
    ids = g.dirty_patches(d.data_ptr())
    dplan = g.plan_dirty(d.data_ptr(), problem=1)
    assert np.array_equal(dplan.gids, ids + NP)
    torch.cuda.synchronize()
    dplan.execute(b.data_ptr() + 8 * mstride, q.data_ptr() + 8 * mstride)        # on member 1's slab
    dplan.status()
    g.lod_matrix_update(d.data_ptr(), b.data_ptr() + 8 * mstride, q.data_ptr() + 8 * mstride, stride, V.data_ptr() + 8, ld_m=ld)
    torch.cuda.synchronize()
    W = _nan(NP * cap, ld)
    g.lod_matrix_ensemble(b.data_ptr(), q.data_ptr(), stride, K, W.data_ptr(), cols.data_ptr(), ld_m=ld)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(V), _bits(W))
    assert np.array_equal(_bits(V[:, [0, 2, 3, 4]]), _bits(old[:, [0, 2, 3, 4]]))
    changed = _bits(V[:, 1]) != _bits(old[:, 1])
    hc = cols.cpu().numpy().view(np.uint32)
    f = _flags(d) != 0
    assert changed.any() and not (changed & ~(np.repeat(f, cap) | f[np.where(hc != 0xffffffff, hc, 0)])).any()


# ---- 4. the mass update

def _mass(c, basis, rho):
    torch, dev = _torch()
    NP, cap, s = c.g.num_patches, c.g.lod_row_capacity(), c.s
    values = _nan(NP * cap * s * s)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    c.g.lod_mass_matrix(np.arange(NP), basis.data_ptr(), c.stride, values.data_ptr(), cols.data_ptr(),
                        d_rho=None if rho is None else rho.data_ptr())
    torch.cuda.synchronize()
    return values


@pytest.mark.parametrize("density", ["one", "random"])
@pytest.mark.parametrize("name", NAMES)
def test_mass_update_equals_fresh_mass_matrix(so, name, density):
    torch, dev = _torch()
    c = _scenario(so, name)
    g = c.g
    rho = None
    if density == "random":
        gen = torch.Generator(device="cpu").manual_seed(17)
        rho = (torch.rand(g.NE * g.NE, generator=gen, dtype=torch.float64) + 0.5).to(dev)
    rp = None if rho is None else rho.data_ptr()
    M0, Mref = _mass(c, c.b0, rho), _mass(c, c.b1, rho)
    assert not np.array_equal(_bits(M0), _bits(Mref))
    M1 = M0.clone()
    torch.cuda.synchronize()
    g.lod_mass_matrix_update(c.dirty.data_ptr(), c.b1.data_ptr(), c.stride, M1.data_ptr(), d_rho=rp)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(M1), _bits(Mref)), (name, density)
    M = _rows_to_dense(g, M1.cpu().numpy(), c.hcols.ravel(), c.s)
    assert np.array_equal(M, M.T)
    S = _sentinel_like(M0)
    torch.cuda.synchronize()
    g.lod_mass_matrix_update(c.dirty.data_ptr(), c.b1.data_ptr(), c.stride, S.data_ptr(), d_rho=rp)
    torch.cuda.synchronize()
    _assert_exactly_the_dirty_entries(c, S, Mref, (name, density))
    none = _zero_dirty(g)
    S = _sentinel_like(M0)
    torch.cuda.synchronize()
    g.lod_mass_matrix_update(none.data_ptr(), c.b1.data_ptr(), c.stride, S.data_ptr(), d_rho=rp)
    torch.cuda.synchronize()
    assert (_bits(S) == SENTINEL).all()
    every = torch.full_like(none, 1)
    M = M0.clone()
    torch.cuda.synchronize()
    g.lod_mass_matrix_update(every.data_ptr(), c.b1.data_ptr(), c.stride, M.data_ptr(), d_rho=rp)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(M), _bits(Mref))


# ---- 5. end to end

def test_refreshed_system_solves_like_a_full_rebuild(so):
    """step64: refreshed slabs and matrix -> C^T f -> slod_lod_solve -> C u_H equals the pipeline on a full rebuild,
    word for word"""
    torch, dev = _torch()
    c = _scenario(so, "step64")
    g, NP = c.g, c.g.num_patches
    Af, _ = _lod_matrix(g, c.bf, c.qf, c.stride, c.s)
    load = torch.zeros((g.NE + 1) ** 2, dtype=torch.float64, device=dev)
    g.fem_rhs(None, load.data_ptr())
    torch.cuda.synchronize()

    def pipeline(b, A):
        rhs, u, fine = _nan(NP), _nan(NP), _nan((g.NE + 1) ** 2)
        torch.cuda.synchronize()
        g.lod_rhs(np.arange(NP), b.data_ptr(), c.stride, load.data_ptr(), rhs.data_ptr())
        it, res = g.lod_solve(A.data_ptr(), c.cols.data_ptr(), rhs.data_ptr(), u.data_ptr(), 1e-13, 5000)
        g.lod_reconstruct(b.data_ptr(), c.stride, u.data_ptr(), fine.data_ptr())
        torch.cuda.synchronize()
        return u, it, res, fine

    u1, it1, res1, fine1 = pipeline(c.b1, c.A1)
    uf, itf, resf, finef = pipeline(c.bf, Af)
    u0, _, _, _ = pipeline(c.b0, c.A0)
    assert it1 == itf and it1 > 0 and res1 <= 1e-12
    assert np.array_equal(_bits(u1), _bits(uf)) and np.array_equal(_bits(fine1), _bits(finef))
    assert not np.array_equal(_bits(u1), _bits(u0))


# ---- 6. the driver

def test_driver_perturb_refresh_matches_rebuild():
    """bin/main_Diffusion 3 4 1 1 --perturb 2: two cells of the 8 x 8 coefficient grid flip, the basis and A_LOD are
    refreshed in place, and a second problem is built from scratch on the changed coefficient.  The dirty list holds
    clipped patches and the rebuild goes through the host-buffer path, so the two need not agree bit for bit: A_LOD to
    the 1e-12 of its scale of the dense-matrix test of test_gpu_lod_system.py, u_H to the 1e-8 of its scale that test
    allows the coarse solve."""
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "4", "1", "1", "--perturb", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    m = re.search(r"^perturbation of 2 coefficient cells: dirty patches = (\d+) of (\d+)$", r.stdout, re.M)
    assert m, r.stdout
    n_dirty, n_patches = int(m.group(1)), int(m.group(2))
    # a cell of the 8 x 8 coefficient grid is a coarse cell here; the generator picks (4, 3), which 3 x 3 patches see, and
    # (2, 7) on the upper edge, which 3 x 2 others see
    assert n_patches == 64 and n_dirty == 15
    a = re.search(r"max \|A_refresh - A_rebuild\| = (\S+) +\(max \|A_rebuild\| = (\S+)\)", r.stdout)
    u = re.search(r"max \|u_refresh - u_rebuild\| = (\S+) +\(max \|u_rebuild\| = (\S+)\)", r.stdout)
    assert a and u, r.stdout
    assert float(a.group(2)) > 0.0 and float(u.group(2)) > 0.0
    assert float(a.group(1)) <= 1e-12 * float(a.group(2)), a.group(0)
    assert float(u.group(1)) <= 1e-8 * float(u.group(2)), u.group(0)
    # without the option nothing of it is printed
    plain = subprocess.run([BIN, "3", "4", "1", "1"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "perturbation" not in plain.stdout
