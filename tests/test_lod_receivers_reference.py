"""The yardstick of the receivers (lod_receiver_cases) checked on a machine without a GPU, on the five geometries of
lod_cases.SLAB_CONFIGS with the oracle's patch extents and random slabs (non-zero on rims, NaN in every gap): its rows
times a random u are the reference reconstruction at every node and component; the entry counts are those of the covering
closed patches; the library's host-only slod_lod_receiver_pattern gives the yardstick's columns; and the bilinear terms of
a point reproduce a bilinear function."""
import numpy as np
import pytest

import lod_receiver_cases as rc
from lod_cases import SLAB_CONFIGS, _layout_geometry, _mk, _random_slab, _ref_reconstruct, _slab_bar

GEOMS = tuple(SLAB_CONFIGS)


def _geom(so, name):
    kw = SLAB_CONFIGS[name]
    cfg = so.make_cfg(**kw)
    return _layout_geometry(kw, lambda p: so.patch_info(cfg, p))


def _full_stride(geom):
    return geom.s * geom.s * (geom.n * (2 * geom.l + 1) + 1) ** 2


@pytest.mark.parametrize("name", GEOMS)
def test_rows_times_u_equal_the_reference_reconstruction(so, name):
    geom = _geom(so, name)
    stride = _full_stride(geom) + 3
    slab, (Phi,) = _random_slab(geom, stride, 31)
    u = np.random.default_rng(32).uniform(-1.0, 1.0, geom.NP * geom.s)
    ref, sabs, m = _ref_reconstruct(geom, Phi, u)
    got = np.zeros((geom.NEp * geom.NEp, geom.s))
    cnt = np.zeros((geom.NEp * geom.NEp, geom.s), dtype=np.int64)
    for node in range(geom.NEp * geom.NEp):
        cols = rc.term_columns(geom, node)
        for c in range(geom.s):
            off = rc.term_offsets(geom, node, c, stride)
            vals = rc.term_values(geom, Phi, node, c)
            assert np.array_equal(slab[off], vals) and np.isfinite(vals).all()       # the offsets point at the same words
            got[node, c] = np.dot(vals, u[cols])
            cnt[node, c] = len(cols)
            y, s_abs, mm = rc.receiver_value(geom, Phi, [(node, c, 1.0)], u)
            assert mm == len(cols) and abs(y - ref.reshape(-1, geom.s)[node, c]) <= 4 * 2.0 ** -64 * max(s_abs, 1e-300) * mm
    ok, worst = _slab_bar(got.reshape(ref.shape), ref, sabs, m)
    assert ok, (name, worst)
    assert np.array_equal(cnt.reshape(m.shape), m)        # the terms of the reference sum: one per covering patch and d


@pytest.mark.parametrize("name", GEOMS)
def test_entry_counts(so, name):
    geom = _geom(so, name)
    n, l, s, N = geom.n, geom.l, geom.s, geom.N
    cap = (2 * l + 2) ** 2 * s
    for node in range(geom.NEp * geom.NEp):
        cnt = len(rc.term_columns(geom, node))
        assert cnt == rc.covering_patches(geom, node) * s and 0 < cnt <= cap
        X, Y = node % geom.NEp, node // geom.NEp
        # (2 l + 2)^2 patches: 2 l + 2 centre cells in x and in y, which takes a coarse-cell corner with l + 1 cells on
        # either side
        far = all(v % n == 0 and l + 1 <= v // n <= N - l - 1 for v in (X, Y))
        assert (cnt == cap) == far, (name, node)
        if name == "whole":
            assert cnt == geom.NP * s


@pytest.mark.parametrize("name", ("rowmajor", "whole", "wide", "mixed"))
def test_library_pattern_equals_the_yardstick(so, name):
    geom = _geom(so, name)
    _, g = _mk(so, stabilize=1, **SLAB_CONFIGS[name])
    cap = g.lod_receiver_capacity()
    assert cap == (2 * geom.l + 2) ** 2 * geom.s
    for node in range(geom.NEp * geom.NEp):
        got = g.lod_receiver_pattern(node)
        assert len(got) <= cap and np.array_equal(got, rc.term_columns(geom, node)), (name, node)
    import slod_amd
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_receiver_pattern(geom.NEp * geom.NEp)
    assert e.value.code == -1 and "slod_lod_receiver_pattern: node out of range" in str(e.value)


def test_point_terms():
    import slod_amd
    NE, rng = 12, np.random.default_rng(7)
    a, b, c, d = rng.uniform(-0.25, 0.25, 4)              # |f| <= 1 on the unit square
    NEp = NE + 1
    yy, xx = np.meshgrid(np.arange(NEp) / NE, np.arange(NEp) / NE, indexing="ij")
    f = (a + b * xx + c * yy + d * xx * yy).ravel()        # bilinear: the Q1 interpolant is the function
    for x, y in rng.uniform(0.0, 1.0, (50, 2)):
        terms = slod_amd.point_terms(NE, 1, x, y, 0)
        w = np.array([t[2] for t in terms])
        assert len(terms) == 4 and abs(w.sum() - 1.0) <= 4e-16 and (w >= 0.0).all()
        val = sum(t[2] * f[t[0]] for t in terms)
        assert abs(val - (a + b * x + c * y + d * x * y)) <= 1e-15
        mine = rc.point_terms(NE, x, y, 0)
        assert [t[0] for t in mine] == [t[0] for t in terms] and np.allclose(w, [t[2] for t in mine], rtol=0, atol=1e-15)
    NE, NEp = 16, 17                                        # x NE is exact
    for ix, iy in ((0, 0), (5, 7), (NE, 3), (4, NE), (NE, NE)):
        terms = slod_amd.point_terms(NE, 2, ix / NE, iy / NE, 1)
        assert [t[2] for t in terms] == [1.0, 0.0, 0.0, 0.0] and terms[0][:2] == (ix + iy * NEp, 1)
        assert all(0 <= t[0] < NEp * NEp for t in terms)
    for bad in ((-0.1, 0.5, 0), (0.5, 1.5, 0), (0.5, 0.5, 2)):
        with pytest.raises(ValueError):
            slod_amd.point_terms(NE, 2, *bad)
