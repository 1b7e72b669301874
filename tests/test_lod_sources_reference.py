"""The yardstick of the sources (lod_source_cases) checked on a machine without a GPU, on the five geometries of
lod_cases.SLAB_CONFIGS with the oracle's patch extents and random slabs: b = O^T g of the six sources in np.longdouble
against O_dense^T g, and against the reference C^T f (lod_cases._ref_rhs) of the fine field f = sum w e(node, c) g that the
sources stand for; the transposed index against a direct scan; slod_amd.ricker against its closed form."""
import numpy as np
import pytest

import lod_receiver_cases as rc
import lod_source_cases as sc
from lod_cases import SLAB_CONFIGS, U53, _layout_geometry, _random_slab, _ref_rhs, _slab_bar

GEOMS = tuple(SLAB_CONFIGS)


def _geom(so, name):
    kw = SLAB_CONFIGS[name]
    cfg = so.make_cfg(**kw)
    return _layout_geometry(kw, lambda p: so.patch_info(cfg, p))


def _case(so, name):
    geom = _geom(so, name)
    stride = geom.s * geom.s * (geom.n * (2 * geom.l + 1) + 1) ** 2 + 3
    _, (Phi,) = _random_slab(geom, stride, 31)
    sources = sc.six(geom.n, geom.N, geom.s)
    return geom, Phi, sources, rc.receiver_rows(geom, Phi, sources)


@pytest.mark.parametrize("name", GEOMS)
def test_yardstick_against_dense_rows_and_the_reference_load(so, name):
    geom, Phi, sources, (rb, cols, vals) = _case(so, name)
    nrow = geom.NP * geom.s
    rng = np.random.default_rng(33)
    g = rng.uniform(-1.0, 1.0, (len(sources), 3))
    base = rng.uniform(-1.0, 1.0, (nrow, 3))
    b, sabs, m = sc.inject_value(rb, cols, vals, g, nrow, base)
    b0, sabs0, m0 = sc.inject_value(rb, cols, vals, g, nrow)
    # the densified rows: the same sum in float64, other order
    O = sc.dense_rows(rb, cols, vals, nrow)
    ok, worst = _slab_bar(base + O.T @ g, b, sabs, m)
    assert ok, (name, worst)
    ok, worst = _slab_bar(O.T @ g, b0, sabs0, m0)
    assert ok, (name, worst)
    touched = np.zeros(nrow, dtype=bool)
    touched[cols] = True
    assert np.array_equal(m[:, 0] - 1, np.bincount(cols, minlength=nrow)) and (b0[~touched] == 0).all()
    assert np.array_equal(b[~touched].astype(np.float64), base[~touched])
    # the fine field the sources stand for, through the reference C^T f; the values w phi of the rows are rounded once, which
    # is one of the + 16 of the bar
    for col in range(3):
        F = np.zeros((geom.NEp * geom.NEp, geom.s), dtype=np.longdouble)
        for q, terms in enumerate(sources):
            for node, comp, w in terms:
                F[node, comp] += np.longdouble(w) * np.longdouble(g[q, col])
        ref, rabs, rm = _ref_rhs(geom, Phi, F)
        err = np.abs(b0[:, col] - ref)
        assert (err <= (m0[:, col] + 16) * np.longdouble(U53) * np.maximum(sabs0[:, col], rabs)).all(), (name, col)
        assert (ref[~touched] == 0).all()


@pytest.mark.parametrize("name", GEOMS)
def test_transposed_index(so, name):
    geom, Phi, sources, (rb, cols, vals) = _case(so, name)
    nrow = geom.NP * geom.s
    rows, begin, perm, q, slot = sc.transposed_index(rb, cols, nrow)
    assert np.array_equal(rows, sorted(set(int(c) for c in cols))) and begin[-1] == len(cols) == len(perm)
    src_of = [k for k in range(len(sources)) for _ in range(int(rb[k]), int(rb[k + 1]))]
    for t, r in enumerate(rows):
        es = [e for e in range(len(cols)) if cols[e] == r]                 # ascending e
        assert list(perm[begin[t]:begin[t + 1]]) == es and list(q[begin[t]:begin[t + 1]]) == [src_of[e] for e in es]
        assert slot[r] == t
    assert (slot >= 0).sum() == len(rows) and set(slot[slot < 0]) <= {-1}
    # the 4-term point repeats coarse columns inside a source; two sources share coarse rows
    inside = cols[rb[4]:rb[5]]
    assert len(set(inside.tolist())) < len(inside)
    assert set(cols[rb[0]:rb[1]].tolist()) & set(cols[rb[5]:rb[6]].tolist())
    assert min(t[2] for s in sources for t in s) < 0.0


def test_ricker():
    import slod_amd
    f0, t0 = 12.5, 0.11
    t = np.array([0.0, 0.05, t0, t0 + np.sqrt(6.0) / (2.0 * np.pi * f0), 0.3])
    w = slod_amd.ricker(t, f0, t0, amp=-2.5)
    assert w.dtype == np.float64 and w.shape == t.shape
    for x, y in zip(t, w):
        ref = sc.ricker_closed(float(x), f0, t0, -2.5)
        assert abs(y - ref) <= 8 * 2.0 ** -53 * max(abs(ref), 2.5 * np.exp(-1.5) * 2)
    assert w[2] == -2.5                                                 # the peak, at t0
    # the zeros at t0 +- 1 / (sqrt(2) pi f0), the minimum -2 e^(-3/2) amp at t0 +- sqrt(6) / (2 pi f0)
    assert abs(slod_amd.ricker(t0 + 1.0 / (np.sqrt(2.0) * np.pi * f0), f0, t0)) <= 1e-15
    assert abs(slod_amd.ricker(t[3], f0, t0) + 2.0 * np.exp(-1.5)) <= 1e-15
    assert slod_amd.ricker(0.0, f0, t0) == slod_amd.ricker(2 * t0, f0, t0)   # even about t0
