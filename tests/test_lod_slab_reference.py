"""The references of the slab consumers (lod_cases._ref_matrix, _ref_mass, _ref_rhs, _ref_reconstruct) checked on a
machine without a GPU, on every geometry test_gpu_lod_slabs.py runs and with the oracle's patch extents: against the
dense scatter of every patch vector to the global fine grid (the construction of lod_cases._global_dense, on plain
extents), against the fine Q1 mass, and against the all-ones counts the reference project prints."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from lod_cases import (SLAB_CONFIGS, UNUSED, _layout_geometry, _mass_fine, _random_slab, _ref_mass, _ref_matrix, _ref_reconstruct,
                       _ref_rhs, _rim_mask, _slot_columns)

GEOMS = tuple(SLAB_CONFIGS)
REL = 1e-13


def _geom(so, name):
    kw = SLAB_CONFIGS[name]
    cfg = so.make_cfg(**kw)
    assert so.num_patches(cfg) == so.n_cells_per_side(cfg) ** 2
    return _layout_geometry(kw, lambda p: so.patch_info(cfg, p))


def _full_stride(geom):
    return geom.s * geom.s * (geom.n * (2 * geom.l + 1) + 1) ** 2


def _scatter(geom, vecs):
    """[(NP s)][(NEp^2 s)]: row (p, d) is the vector phi_{p,d} on the global fine grid, zero outside the patch."""
    n, s, NEp = geom.n, geom.s, geom.NEp
    out = np.zeros((geom.NP * s, NEp * NEp * s))
    for p in range(geom.NP):
        x0, y0, mx, my = geom.ext[p]
        for d in range(s):
            G = out[p * s + d].reshape(NEp, NEp, s)
            G[y0 * n:(y0 + my) * n + 1, x0 * n:(x0 + mx) * n + 1, :] = vecs[p][d]
    return out


def _as_matrix(geom, blocks):
    """[NP][NP][s][s] -> [(NP s)][(NP s)]"""
    return np.asarray(blocks, dtype=np.float64).transpose(0, 2, 1, 3).reshape(geom.NP * geom.s, geom.NP * geom.s)


def _close(got, want):
    return np.abs(got - want).max() <= REL * np.abs(want).max()


@pytest.mark.parametrize("name", GEOMS)
def test_random_slab_layout(so, name):
    """Patch p of member k starts at k member_stride + p stride, its s vectors follow each other, and every other word
    is NaN; the values do not depend on the stride."""
    geom = _geom(so, name)
    stride = _full_stride(geom)
    assert stride >= geom.s * geom.n_fine.max()
    slab, vecs = _random_slab(geom, stride + 5, 11, members=2, member_gap=7)
    _, again = _random_slab(geom, stride, 11, members=2)
    mstride = geom.NP * (stride + 5) + 7
    seen = np.zeros(slab.size, dtype=bool)
    for k in range(2):
        for p in range(geom.NP):
            off, cnt = k * mstride + p * (stride + 5), geom.s * geom.n_fine[p]
            assert np.array_equal(slab[off:off + cnt], vecs[k][p].ravel()) and np.array_equal(vecs[k][p], again[k][p])
            seen[off:off + cnt] = True
    assert np.isnan(slab[~seen]).all() and (~seen).sum() == 2 * (geom.NP * (stride + 5) + 7) - 2 * geom.s * geom.n_fine.sum()


@pytest.mark.parametrize("name", GEOMS)
def test_references_equal_the_dense_scatter(so, name):
    geom = _geom(so, name)
    _, (Phi,) = _random_slab(geom, _full_stride(geom), 1)
    _, (Psi,) = _random_slab(geom, _full_stride(geom), 2)
    rng = np.random.default_rng(3)
    f, u = rng.uniform(-1.0, 1.0, geom.field), rng.uniform(-1.0, 1.0, geom.NP * geom.s)
    DPhi, DPsi = _scatter(geom, Phi), _scatter(geom, Psi)
    ref, sabs, m, shared = _ref_matrix(geom, Phi, Psi)
    dense = DPhi @ DPsi.T
    assert _close(_as_matrix(geom, ref), dense)
    assert (np.abs(ref) <= sabs).all() and _close(_as_matrix(geom, sabs), np.abs(DPhi) @ np.abs(DPsi).T)
    # the pattern is the support of |Phi| |Psi|^T, and m counts its products
    count = (DPhi != 0).astype(np.float64) @ (DPsi != 0).astype(np.float64).T
    assert np.array_equal(count[::geom.s, ::geom.s] > 0, shared) and np.array_equal(count[::geom.s, ::geom.s], m)
    rref, rabs, rm = _ref_rhs(geom, Phi, f)
    assert _close(np.asarray(rref, dtype=np.float64), DPhi @ f) and (np.abs(rref) <= rabs).all()
    assert np.array_equal(rm, np.repeat(geom.n_fine, geom.s))
    cref, cabs, cm = _ref_reconstruct(geom, Phi, u)
    assert _close(np.asarray(cref, dtype=np.float64).ravel(), DPhi.T @ u) and (np.abs(cref) <= cabs).all()
    assert np.array_equal(cm.ravel(), (DPhi != 0).sum(axis=0)) and cm.min() >= geom.s
    # the slots of a block row hold every coupled patch once
    cols = _slot_columns(geom, shared)
    for p in range(geom.NP):
        assert sorted(int(q) for q in cols[p] if q != UNUSED) == [int(q) for q in np.nonzero(shared[p])[0]]


@pytest.mark.parametrize("density", ["one", "random"])
@pytest.mark.parametrize("name", GEOMS)
def test_mass_reference_with_zero_rims_is_the_fine_mass(so, name, density):
    """With phi = 0 on every patch rim the sum over the intersection rectangles is the global form Phi M_h Phi^T."""
    geom = _geom(so, name)
    _, (Phi,) = _random_slab(geom, _full_stride(geom), 4)
    for v in Phi:
        v[:, _rim_mask(v.shape[1], v.shape[2]), :] = 0.0
    rho = None if density == "one" else np.random.default_rng(5).uniform(0.5, 2.0, geom.NE * geom.NE)
    ref, sabs, m, shared = _ref_mass(geom, Phi, rho)
    D = _scatter(geom, Phi)
    Mh = np.kron(_mass_fine(geom.NE, rho), np.eye(geom.s))
    dense = D @ Mh @ D.T
    assert np.abs(dense).max() > 0.0 and _close(_as_matrix(geom, ref), dense)
    assert (np.abs(ref) <= sabs).all()


@pytest.mark.parametrize("density", ["one", "random"])
@pytest.mark.parametrize("name", GEOMS)
def test_mass_reference_all_ones_counts_elements(so, name, density):
    """phi = 1 everywhere: every entry of the pair (p, q) is s h^2 sum of rho over the elements of the intersection, and
    the row sums are the formula of test_mass_matrix_all_ones_counts_elements."""
    geom = _geom(so, name)
    n, s, NE = geom.n, geom.s, geom.NE
    ones = [np.ones((s, geom.ext[p, 3] * n + 1, geom.ext[p, 2] * n + 1, s)) for p in range(geom.NP)]
    rho = np.ones(NE * NE) if density == "one" else np.random.default_rng(6).uniform(0.5, 2.0, NE * NE)
    ref, sabs, m, shared = _ref_mass(geom, ones, None if density == "one" else rho)
    assert np.array_equal(ref, sabs)
    r2 = rho.reshape(NE, NE)
    mult = np.zeros((NE, NE))
    for p in range(geom.NP):
        x0, y0, mx, my = geom.ext[p]
        mult[y0 * n:(y0 + my) * n, x0 * n:(x0 + mx) * n] += 1.0
        for q in range(geom.NP):
            xa, xb = max(x0, geom.ext[q, 0]) * n, min(x0 + mx, geom.ext[q, 0] + geom.ext[q, 2]) * n
            ya, yb = max(y0, geom.ext[q, 1]) * n, min(y0 + my, geom.ext[q, 1] + geom.ext[q, 3]) * n
            want = s * r2[ya:max(yb, ya), xa:max(xb, xa)].sum() / (NE * NE)
            assert np.abs(np.asarray(ref[p, q], dtype=np.float64) - want).max() <= REL * max(want, 1e-300), (p, q)
            assert m[p, q] == s * max(xb - xa, 0) * max(yb - ya, 0)
    weight = r2 * mult / (NE * NE)
    for p in range(geom.NP):
        x0, y0, mx, my = geom.ext[p]
        want = s * weight[y0 * n:(y0 + my) * n, x0 * n:(x0 + mx) * n].sum()
        for d in range(s):
            assert abs(float(ref[p, :, d, d].sum()) - want) <= REL * want


def test_matrix_reference_all_ones_is_the_parallel_assembly_golden(so):
    """The all-ones slab on the golden geometry: the 1024 entries the reference project prints (2 x shared fine nodes)."""
    geom = _geom(so, "golden")
    ones = [np.ones((2, geom.ext[p, 3] * 2 + 1, geom.ext[p, 2] * 2 + 1, 2)) for p in range(geom.NP)]
    ref, sabs, m, shared = _ref_matrix(geom, ones, ones)
    A = _as_matrix(geom, ref)
    assert np.array_equal(ref, sabs) and np.array_equal(ref[:, :, 0, 0], m)
    k = 0
    for ln in open(os.path.join(GOLDEN, "reference", "parallel_assembly.output")).read().split("\n"):
        if ln.startswith("("):
            ij, val = ln.split(")")
            i, j = (int(x) for x in ij[1:].split(","))
            assert A[i, j] == float(val), (i, j)
            k += 1
    assert k == 1024
