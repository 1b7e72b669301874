"""GPU tests of the receivers on the LOD space (slod_lod_receivers_create, slod_lod_observe_multi / _ensemble) on the
random slabs of lod_cases.SLAB_CONFIGS: every word of every patch vector random, rims included, and NaN wherever nothing
must be read (between s n_fine(p) and the stride, between the members, in the padding of every multi-vector); every
test runs with the stride of an empty plan and with stride + 5.

The yardstick is equality of 64-bit words: the rows against the slab's words (lod_receiver_cases), the product of a
one-term receiver of weight 1 against slod_lod_reconstruct_multi / _ensemble at that node and component.  Receivers of
several terms are compared with the np.longdouble value within lod_cases._slab_bar, (m + 16) 2^-53 S_abs: derived, not
tuned; the worst ratio is printed."""
import numpy as np
import pytest

import lod_receiver_cases as rc
from lod_cases import NAN, SLAB_CONFIGS, _Case, _bits, _layout_geometry, _mk, _random_slab, _slab_bar, _torch

pytestmark = pytest.mark.gpu

GEOMS = tuple(SLAB_CONFIGS)
PADS = (0, 5)
K = 3
_setups, _devs = {}, {}


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _nan(*shape):
    torch, dev = _torch()
    return torch.full(shape, NAN, dtype=torch.float64, device=dev)


def _sync():
    _torch()[0].cuda.synchronize()


def _setup(so, name, pad):
    """Handle, geometry, one-member and K-member slabs on the device and their host vectors; once per (geometry, pad)."""
    if (name, pad) not in _devs:
        if name not in _setups:
            c = _Case()
            kw = SLAB_CONFIGS[name]
            _, c.g = _mk(so, stabilize=1, **kw)
            c.name, c.geom = name, _layout_geometry(kw, c.g.patch_layout)
            c.s, c.NP, c.nnode = c.geom.s, c.geom.NP, c.geom.NEp ** 2
            c.stride0 = c.g.plan(np.zeros(0, dtype=np.uint32)).stride
            c.nodes = np.arange(c.nnode) if name != "mixed" else rc.sample_nodes(c.geom, 64)
            _setups[name] = c
        c = _setups[name]
        d = _Case()
        d.stride = c.stride0 + pad
        d.mstride = c.NP * d.stride + 7
        hb, d.Phi = _random_slab(c.geom, d.stride, 21)
        he, d.PhiK = _random_slab(c.geom, d.stride, 61, members=K, member_gap=7)
        d.b, d.e = _dev(hb), _dev(he)
        _devs[(name, pad)] = d
    return _setups[name], _devs[(name, pad)]


def _nodal(c, nodes, weight=1.0):
    """One receiver per (node, component), node-major: receiver index = position of the node * s + component."""
    return [[(int(nd), comp, weight)] for nd in nodes for comp in range(c.s)]


def _reconstruct_multi(c, d, U, n_rhs):
    fine = _nan(n_rhs, c.geom.field + 3)
    c.g.lod_reconstruct_multi(d.b.data_ptr(), d.stride, U.data_ptr(), U.shape[1], n_rhs, fine.data_ptr(), fine.shape[1])
    _sync()
    return fine


def _pick(c, fine, nodes):
    """[len(nodes) s][columns] words of a field-major fine multi-vector at the nodes, in the order of _nodal."""
    idx = (np.asarray(nodes)[:, None] * c.s + np.arange(c.s)[None, :]).ravel()
    return _bits(fine[:, :c.geom.field]).T[idx]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_rows(so, name, pad):
    """Weight 1: the values are the slab's words; weight w: w phi rounded once; columns and row_begin equal the yardstick;
    everything is finite although the slab is NaN between vectors, strides and members; K = 3: member-minor, member m
    equals a one-member object on member m's slab as words."""
    c, d = _setup(so, name, pad)
    g, geom = c.g, c.geom
    point = rc.point_terms(geom.NE, 0.37, 0.61, c.s - 1)
    recs = _nodal(c, c.nodes) + _nodal(c, c.nodes[:7], -0.3) + [point, [(0, 0, 2.5), (int(c.nodes[-1]), c.s - 1, -2.5)]]
    R = g.lod_receivers(recs, d.b.data_ptr(), d.stride)
    rb, cols, vals = R.rows()
    wrb, wcols, wvals = rc.receiver_rows(geom, d.Phi[0], recs)
    assert np.array_equal(rb, wrb) and np.array_equal(cols, wcols)
    assert np.isfinite(vals).all() and np.array_equal(vals.view(np.uint64), wvals.view(np.uint64))
    n1 = int(rb[len(c.nodes) * c.s])                                       # the weight-1 rows: plain words of the slab
    off = np.concatenate([rc.term_offsets(geom, t[0][0], t[0][1], d.stride) for t in recs[:len(c.nodes) * c.s]])
    assert np.array_equal(vals[:n1].view(np.uint64), d.b.cpu().numpy()[off].view(np.uint64))
    assert (R.info.n_receivers, R.info.n_members, R.info.nnz) == (len(recs), 1, len(cols))
    assert R.info.bytes == 8 * len(cols) + 4 * (len(cols) + len(recs) + 1)
    assert max(len(g.lod_receiver_pattern(int(nd))) for nd in c.nodes) <= g.lod_receiver_capacity()
    # ensemble slab
    RK = g.lod_receivers(recs, d.e.data_ptr(), d.stride, n_members=K, member_stride=d.mstride)
    assert (RK.info.n_members, RK.info.nnz) == (K, len(cols))
    for m in range(K):
        rbm, colsm, valsm = RK.rows(m)
        one = g.lod_receivers(recs, d.e.data_ptr() + 8 * m * d.mstride, d.stride)
        _, _, v1 = one.rows()
        want = rc.receiver_rows(geom, d.PhiK[m], recs)[2]
        assert np.array_equal(rbm, wrb) and np.array_equal(colsm, wcols)
        assert np.array_equal(valsm.view(np.uint64), v1.view(np.uint64)) and np.array_equal(v1.view(np.uint64), want.view(np.uint64))
        one.close()
    R.close(), RK.close()


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_observe_equals_reconstruct_multi(so, name, pad):
    """All nodal receivers at once (mixed: a 64-node sample with corners, edges, cell corners and interiors): y has the
    words of slod_lod_reconstruct_multi at n_rhs 1, 3 and 65; padded ld_u / ld_y with NaN left untouched; a repeated call;
    the bits of a column do not depend on n_rhs or on its position."""
    torch, dev = _torch()
    c, d = _setup(so, name, pad)
    g = c.g
    R = g.lod_receivers(_nodal(c, c.nodes), d.b.data_ptr(), d.stride)
    nq = len(c.nodes) * c.s
    hu = np.random.default_rng(41).uniform(-1.0, 1.0, (c.NP * c.s, 65))
    first = None
    for n_rhs, ld_u, ld_y in ((1, 1, 1), (3, 5, 4), (65, 65, 67)):
        U = _nan(c.NP * c.s, ld_u)
        U[:, :n_rhs] = _dev(hu[:, :n_rhs])
        Y = _nan(nq + 2, ld_y)
        R.observe(U.data_ptr(), Y.data_ptr(), n_rhs=n_rhs, ld_u=ld_u, ld_y=ld_y)
        _sync()
        want = _pick(c, _reconstruct_multi(c, d, U, n_rhs), c.nodes)
        assert np.array_equal(_bits(Y[:nq, :n_rhs]), want), (name, n_rhs)
        assert bool(torch.isnan(Y[:nq, n_rhs:]).all()) and bool(torch.isnan(Y[nq:]).all())
        again = _nan(nq + 2, ld_y)
        R.observe(U.data_ptr(), again.data_ptr(), n_rhs=n_rhs, ld_u=ld_u, ld_y=ld_y)
        _sync()
        assert np.array_equal(_bits(again), _bits(Y))
        if first is None:
            first = _bits(Y[:nq, 0]).copy()
        assert np.array_equal(_bits(Y[:nq, 0]), first)                    # column 0 whatever n_rhs
    # position: column 0 of hu placed as column 2 of 3
    U = _dev(np.stack([hu[:, 7], hu[:, 9], hu[:, 0]], axis=1))
    Y = _nan(nq, 3)
    R.observe(U.data_ptr(), Y.data_ptr(), n_rhs=3)
    _sync()
    assert np.array_equal(_bits(Y[:, 2]), first)
    R.close()


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_observe_equals_reconstruct_ensemble(so, name, pad):
    """K = 3: column m of slod_lod_observe_ensemble has the words of slod_lod_reconstruct_ensemble's field m; a member
    sub-range; NaN padding left untouched."""
    torch, dev = _torch()
    c, d = _setup(so, name, pad)
    g = c.g
    R = g.lod_receivers(_nodal(c, c.nodes), d.e.data_ptr(), d.stride, n_members=K, member_stride=d.mstride)
    nq, ld_u, ld_y = len(c.nodes) * c.s, K + 1, K + 2
    U = _nan(c.NP * c.s, ld_u)
    U[:, :K] = _dev(np.random.default_rng(42).uniform(-1.0, 1.0, (c.NP * c.s, K)))
    fine = _nan(K, c.geom.field + 3)
    g.lod_reconstruct_ensemble(d.e.data_ptr(), d.stride, K, U.data_ptr(), fine.data_ptr(), ld_fine=fine.shape[1],
                               member_stride=d.mstride, ld_u=ld_u)
    Y = _nan(nq + 1, ld_y)
    R.observe_ensemble(U.data_ptr(), Y.data_ptr(), ld_u=ld_u, ld_y=ld_y)
    _sync()
    want = _pick(c, fine, c.nodes)
    assert np.array_equal(_bits(Y[:nq, :K]), want)
    assert bool(torch.isnan(Y[:nq, K:]).all()) and bool(torch.isnan(Y[nq:]).all())
    part = _nan(nq, ld_y)                                                 # members 1 .. K-1 on columns 0 .. K-2
    R.observe_ensemble(U.data_ptr() + 8, part.data_ptr(), n_members=K - 1, first_member=1, ld_u=ld_u, ld_y=ld_y)
    _sync()
    assert np.array_equal(_bits(part[:, :K - 1]), want[:, 1:]) and bool(torch.isnan(part[:, K - 1:]).all())
    R.close()


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", GEOMS)
def test_multi_term_receivers(so, name, pad):
    """Point receivers of 4 terms and a 9-term average against the np.longdouble yardstick within lod_cases._slab_bar."""
    c, d = _setup(so, name, pad)
    g, geom = c.g, c.geom
    rng = np.random.default_rng(43)
    recs = [rc.point_terms(geom.NE, x, y, int(comp)) for (x, y), comp in zip(rng.uniform(0.0, 1.0, (12, 2)), rng.integers(0, c.s, 12))]
    mid = geom.NE // 2
    recs.append([(mid + i + (mid + j) * geom.NEp, 0, 1.0 / 9.0) for j in (-1, 0, 1) for i in (-1, 0, 1)])
    recs.append([(0, 0, 1.0), (geom.NE, c.s - 1, -1.0)])
    R = g.lod_receivers(recs, d.b.data_ptr(), d.stride)
    hu = rng.uniform(-1.0, 1.0, (c.NP * c.s, 2))
    Y = _nan(len(recs), 2)
    R.observe(_dev(hu).data_ptr(), Y.data_ptr(), n_rhs=2)
    _sync()
    got = Y.cpu().numpy()
    ref, sabs = np.zeros(got.shape, dtype=np.longdouble), np.zeros(got.shape, dtype=np.longdouble)
    m = np.zeros(got.shape, dtype=np.int64)
    for q, t in enumerate(recs):
        for col in range(2):
            ref[q, col], sabs[q, col], m[q, col] = rc.receiver_value(geom, d.Phi[0], t, hu[:, col])
    ok, worst = _slab_bar(got, ref, sabs, m)
    print("observe %s stride + %d: worst |got - ref| / bound = %.3f" % (name, pad, worst))
    assert ok, (name, pad, worst)
    R.close()


def test_refusals_that_need_an_object(so):
    import slod_amd
    c, d = _setup(so, "rowmajor", 0)
    g = c.g
    _, other = _mk(so, stabilize=1, **SLAB_CONFIGS["rowmajor"])
    R1 = g.lod_receivers(_nodal(c, c.nodes[:4]), d.b.data_ptr(), d.stride)
    RK = g.lod_receivers(_nodal(c, c.nodes[:4]), d.e.data_ptr(), d.stride, n_members=K, member_stride=d.mstride)
    U, Y = _nan(c.NP * c.s, K), _nan(4, K)
    before = _bits(Y).copy()

    def refused(call, word):
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), str(e.value)

    lib = g.lib
    assert lib.slod_lod_observe_multi(other.h, R1.r, U.data_ptr(), K, K, Y.data_ptr(), K, None) == -1
    assert lib.slod_last_error(other.h).decode() == "slod_lod_observe_multi: receivers of another handle"
    assert lib.slod_lod_observe_ensemble(other.h, RK.r, 0, K, U.data_ptr(), K, Y.data_ptr(), K, None) == -1
    assert lib.slod_last_error(other.h).decode() == "slod_lod_observe_ensemble: receivers of another handle"
    refused(lambda: RK.observe(U.data_ptr(), Y.data_ptr(), n_rhs=K), "slod_lod_observe_multi: receivers of another member count")
    refused(lambda: RK.observe_ensemble(U.data_ptr(), Y.data_ptr(), n_members=K, first_member=1), "members outside the receivers")
    refused(lambda: RK.observe_ensemble(U.data_ptr(), Y.data_ptr(), n_members=1, first_member=-1), "members outside the receivers")
    refused(lambda: R1.observe_ensemble(U.data_ptr(), Y.data_ptr(), n_members=2), "members outside the receivers")
    refused(lambda: R1.observe(U.data_ptr(), Y.data_ptr(), n_rhs=0), "n_rhs < 1")
    refused(lambda: R1.observe(U.data_ptr(), Y.data_ptr(), n_rhs=3, ld_u=2), "leading dimension below n_rhs")
    refused(lambda: R1.observe(U.data_ptr(), Y.data_ptr(), n_rhs=3, ld_y=2), "leading dimension below n_rhs")
    refused(lambda: R1.observe(0, Y.data_ptr()), "NULL")
    refused(lambda: g.lod_receivers((np.array([0, 2, 1, 3]), np.zeros(3), np.zeros(3), np.ones(3)), d.b.data_ptr(), d.stride, raw=True),
            "slod_lod_receivers_create: term_begin does not start at 0 or is not monotone")
    refused(lambda: RK.rows(K), "slod_lod_receivers_rows: member outside the receivers")
    _sync()
    assert np.array_equal(_bits(Y), before)                               # no refused call wrote
    R1.close(), RK.close()
