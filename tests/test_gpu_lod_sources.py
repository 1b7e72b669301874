"""GPU tests of the sources on the LOD space (slod_lod_sources_create, slod_lod_inject_multi / _ensemble) on the real
pencils of lod_cases._pencil (step64: 64 rows, s2: elasticity, 128 rows, rowmajor: 25 rows) and the ensemble
configurations of lod_irk_ensemble_cases (K = 3 and K = 65), with the six sources of lod_source_cases.six.

The yardstick is equality of 64-bit words where the arithmetic is the same: a one-term source of weight 1 and a
power-of-two signal against slod_lod_rhs_multi on the fine field g e(node, c); untouched rows against the base; a column
against its own run; the ensemble against the one-member objects.  Several terms and random signals are compared with the
np.longdouble value of lod_source_cases.inject_value within lod_cases._slab_bar, (m + 16) 2^-53 S_abs with m the entries of
the row plus one for the base: derived, not tuned; the worst ratio is printed ("Sources")."""
import numpy as np
import pytest

import lod_irk_ensemble_cases as ec
import lod_source_cases as sc
from lod_cases import NAN, _bits, _mk, _pencil, _slab_bar, _torch, PENCIL_CONFIGS

pytestmark = pytest.mark.gpu

NAMES = ("step64", "s2", "rowmajor")
SENT_BITS = 0x5a5a5a5a5a5a5a5a
SENT = np.array([SENT_BITS], dtype=np.uint64).view(np.float64)[0]


def _sync():
    _torch()[0].cuda.synchronize()


def _sent(*shape):
    torch, dev = _torch()
    return torch.full(shape, float(SENT), dtype=torch.float64, device=dev)


def _six(c):
    return sc.six(c.g.cfg.n_subdivisions, c.g.N, c.s)


@pytest.mark.parametrize("name", NAMES)
def test_one_term_source_has_the_words_of_the_coarse_load(so, name):
    """Weight 1, signal 1.0, 0.5 and 2.0 on three columns: the touched rows carry the words of slod_lod_rhs_multi on the fine
    field g e(node, c) (every other term of that sum is an exact zero, a power of two commutes with the rounding), the
    other rows +0.0."""
    torch, dev = _torch()
    c = _pencil(so, name)
    g = c.g
    field = (g.NE + 1) ** 2 * c.s
    sig, strongest = np.array([1.0, 0.5, 2.0]), 0.0
    for terms in _six(c)[:4]:
        (node, comp, w), = terms
        R = g.lod_receivers([terms], c.b.data_ptr(), c.stride)
        S = g.lod_sources(R)
        fine = torch.zeros(3, field + 3, dtype=torch.float64, device=dev)
        fine[:, node * c.s + comp] = ec.dev(sig)
        want = ec.nan(c.nrow, 4)
        g.lod_rhs_multi(c.ids, c.b.data_ptr(), c.stride, fine.data_ptr(), fine.shape[1], 3, want.data_ptr(), 4)
        got = _sent(c.nrow, 5)
        G = ec.dev(sig.reshape(1, 3))                                    # named: a temporary's memory may be handed out again
        S.inject(G.data_ptr(), got.data_ptr(), n_rhs=3, ld_b=5)
        _sync()
        rb, cols, vals = R.rows()
        touched = np.zeros(c.nrow, dtype=bool)
        touched[cols] = True
        assert S.info.n_rows_touched == touched.sum() == len(cols) > 0
        assert np.array_equal(_bits(got[:, :3])[touched], _bits(want[:, :3])[touched]), (name, node)
        assert (_bits(got[:, :3])[~touched] == 0).all() and (_bits(got[:, 3:]) == SENT_BITS).all()
        strongest = max(strongest, float(np.abs(got[:, :3].cpu().numpy()[touched]).max()))
        R.close(), S.close()
    assert strongest > 0.0                                                # the basis vanishes at the boundary node, not inside


@pytest.mark.parametrize("name", NAMES)
def test_against_the_longdouble_yardstick(so, name):
    """The six sources, random signals and a random base, 3 columns: within lod_cases._slab_bar of the np.longdouble value."""
    c = _pencil(so, name)
    R = c.g.lod_receivers(_six(c), c.b.data_ptr(), c.stride)
    S = c.g.lod_sources(R)
    rb, cols, vals = R.rows()
    rng = np.random.default_rng(51)
    hg, hb = rng.uniform(-1.0, 1.0, (6, 3)), rng.uniform(-1.0, 1.0, (c.nrow, 3))
    for base in (None, hb):
        got = ec.nan(c.nrow, 3)
        G, B = ec.dev(hg), None if base is None else ec.dev(base)
        S.inject(G.data_ptr(), got.data_ptr(), n_rhs=3, d_base=None if B is None else B.data_ptr())
        _sync()
        ref, sabs, m = sc.inject_value(rb, cols, vals, hg, c.nrow, base)
        ok, worst = _slab_bar(got.cpu().numpy(), ref, sabs, m)
        print("inject %s %s base: worst |got - ref| / bound = %.3f" % (name, "with a" if base is not None else "no", worst))
        assert ok, (name, worst)
    R.close(), S.close()


@pytest.mark.parametrize("name", NAMES)
def test_layout_and_bits(so, name):
    torch, dev = _torch()
    c = _pencil(so, name)
    terms = _six(c)
    if name == "s2":
        terms = terms[1:4]          # on 4 x 4 cells the corner node and the point touch every row: the three on the left
    ns = len(terms)
    R = c.g.lod_receivers(terms, c.b.data_ptr(), c.stride)
    S = c.g.lod_sources(R)
    rb, cols, vals = R.rows()
    touched = np.zeros(c.nrow, dtype=bool)
    touched[cols] = True
    assert 0 < touched.sum() < c.nrow
    rng = np.random.default_rng(52)
    hg, hb = rng.uniform(-1.0, 1.0, (ns, 65)), rng.uniform(-1.0, 1.0, (c.nrow, 65))
    hb[np.flatnonzero(~touched)[0], :] = NAN                              # a NaN in an untouched row travels as it is
    first = None
    for n, ld_g, ld_base, ld_b in ((1, 1, 1, 1), (3, 5, 4, 6), (65, 65, 66, 67)):
        G, B = _sent(ns + 1, ld_g), _sent(c.nrow + 1, ld_base)
        G[:ns, :n], B[:c.nrow, :n] = ec.dev(hg[:, :n]), ec.dev(hb[:, :n])
        out = _sent(c.nrow + 1, ld_b)
        S.inject(G.data_ptr(), out.data_ptr(), n_rhs=n, d_base=B.data_ptr(), ld_g=ld_g, ld_base=ld_base, ld_b=ld_b)
        _sync()
        got = _bits(out)
        assert np.array_equal(got[:c.nrow, :n][~touched], _bits(B)[:c.nrow, :n][~touched])       # the base word, bit for bit
        assert (got[:c.nrow, n:] == SENT_BITS).all() and (got[c.nrow:] == SENT_BITS).all()       # padding untouched
        assert np.isfinite(out[:c.nrow, :n].cpu().numpy()[touched]).all()
        assert not np.array_equal(got[:c.nrow, :n][touched], _bits(B)[:c.nrow, :n][touched])
        nobase = _sent(c.nrow, ld_b)
        S.inject(G.data_ptr(), nobase.data_ptr(), n_rhs=n, ld_g=ld_g, ld_b=ld_b)
        again = _sent(c.nrow + 1, ld_b)                                    # a repeated call
        S.inject(G.data_ptr(), again.data_ptr(), n_rhs=n, d_base=B.data_ptr(), ld_g=ld_g, ld_base=ld_base, ld_b=ld_b)
        inplace = B.clone()                                               # d_b = d_base
        S.inject(G.data_ptr(), inplace.data_ptr(), n_rhs=n, d_base=inplace.data_ptr(), ld_g=ld_g, ld_base=ld_base, ld_b=ld_base)
        _sync()
        assert (_bits(nobase[:, :n])[~touched] == 0).all() and (_bits(nobase[:, n:]) == SENT_BITS).all()
        assert np.array_equal(_bits(again), got)
        assert np.array_equal(_bits(inplace)[:c.nrow, :n], got[:c.nrow, :n]) and (_bits(inplace)[:, n:] == SENT_BITS).all()
        if first is None:
            first = got[:c.nrow, 0].copy()
        assert np.array_equal(got[:c.nrow, 0], first)                     # column 0 whatever the columns and the lds
    # position: column 0 placed as column 2 of 3
    perm = [7, 9, 0]
    out = _sent(c.nrow, 3)
    G, B = ec.dev(hg[:, perm]), ec.dev(hb[:, perm])
    S.inject(G.data_ptr(), out.data_ptr(), n_rhs=3, d_base=B.data_ptr())
    _sync()
    assert np.array_equal(_bits(out[:, 2]), first)
    R.close(), S.close()


@pytest.mark.parametrize("name,K", ec.CASES)
def test_ensemble_equals_multi_per_member(so, name, K):
    """Column m of slod_lod_inject_ensemble has the words of slod_lod_inject_multi on the one-member object of member m; a
    member sub-range on the first columns."""
    c = ec.ens_case(so, name)
    g = c.g
    slab = sc.ens_slab(c, K)
    terms = sc.six(g.cfg.n_subdivisions, g.N, c.s)
    RK = g.lod_receivers(terms, slab.data_ptr(), c.stride, n_members=K, member_stride=c.mstride)
    SK = g.lod_sources(RK)
    assert (SK.info.n_sources, SK.info.n_members) == (6, K)
    rng = np.random.default_rng(53)
    hg, hb = rng.uniform(-1.0, 1.0, (6, K)), rng.uniform(-1.0, 1.0, (c.nrow, K))
    G, B = ec.padded(hg, 1), ec.padded(hb, 2)
    out = _sent(c.nrow, K + 3)
    SK.inject_ensemble(G.data_ptr(), out.data_ptr(), d_base=B.data_ptr(), ld_g=K + 1, ld_base=K + 2, ld_b=K + 3)
    lo, cnt = 1, min(K - 1, 2)
    part = _sent(c.nrow, K + 3)                                            # members lo .. on the columns 0 ..
    SK.inject_ensemble(G.data_ptr() + 8 * lo, part.data_ptr(), n_members=cnt, first_member=lo, d_base=B.data_ptr() + 8 * lo,
                       ld_g=K + 1, ld_base=K + 2, ld_b=K + 3)
    _sync()
    got = _bits(out)
    assert (got[:, K:] == SENT_BITS).all() and (_bits(part)[:, cnt:] == SENT_BITS).all()
    assert np.array_equal(_bits(part)[:, :cnt], got[:, lo:lo + cnt])
    for m in (range(K) if K <= 3 else (0, 1, 2, 3, 31, 63, 64)):
        R1 = g.lod_receivers(terms, slab.data_ptr() + 8 * m * c.mstride, c.stride)
        S1 = g.lod_sources(R1)
        one = _sent(c.nrow, 1)
        G1, B1 = ec.dev(hg[:, m:m + 1]), ec.dev(hb[:, m:m + 1])
        S1.inject(G1.data_ptr(), one.data_ptr(), d_base=B1.data_ptr())
        _sync()
        assert np.array_equal(_bits(one)[:, 0], got[:, m]), (name, K, m)
        R1.close(), S1.close()
    RK.close(), SK.close()


@pytest.mark.parametrize("name", NAMES)
def test_object(so, name):
    """get_info against the transposed index built in numpy; the object survives its receivers."""
    c = _pencil(so, name)
    R = c.g.lod_receivers(_six(c), c.b.data_ptr(), c.stride)
    rb, cols, vals = R.rows()
    S = c.g.lod_sources(R)
    rows, begin, perm, q, slot = sc.transposed_index(rb, cols, c.nrow)
    i = S.info
    assert (i.n_sources, i.n_members, i.n_rows_touched, i.nnz) == (6, 1, len(rows), len(cols))
    assert i.bytes == 8 * len(cols) + 4 * (len(rows) + 1 + len(cols) + c.nrow)
    hg = np.random.default_rng(54).uniform(-1.0, 1.0, (6, 2))
    G = ec.dev(hg)
    a, b = _sent(c.nrow, 2), _sent(c.nrow, 2)
    S.inject(G.data_ptr(), a.data_ptr(), n_rhs=2)
    _sync()
    R.close()
    S.inject(G.data_ptr(), b.data_ptr(), n_rhs=2)
    _sync()
    assert np.array_equal(_bits(a), _bits(b))
    # the chain in the stored order, written out: fma is not in numpy, so within the bar of a sum in that order and exact
    # where a row has one entry and no base (a single rounding)
    ref = np.zeros((c.nrow, 2))
    for t, r in enumerate(rows):
        for k in range(begin[t], begin[t + 1]):
            ref[r] += vals[perm[k]] * hg[q[k]]
    single = np.array([begin[slot[r] + 1] - begin[slot[r]] == 1 if slot[r] >= 0 else True for r in range(c.nrow)])
    assert np.array_equal(_bits(a)[single], ref.view(np.uint64)[single])
    S.close()


def test_refusals_that_need_an_object(so):
    import slod_amd
    c = _pencil(so, "rowmajor")
    g = c.g
    _, other = _mk(so, stabilize=1, **PENCIL_CONFIGS["rowmajor"])
    K = 3
    R1 = g.lod_receivers(_six(c), c.b.data_ptr(), c.stride)
    RK = g.lod_receivers(_six(c), c.b.data_ptr(), c.stride, n_members=K, member_stride=0)
    S1, SK = g.lod_sources(R1), g.lod_sources(RK)
    G, B = ec.nan(6, K), _sent(c.nrow, K)

    def refused(call, word):
        with pytest.raises(slod_amd.SlodError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), str(e.value)

    lib = g.lib
    out = slod_amd.C.c_void_p()
    assert lib.slod_lod_sources_create(other.h, R1.r, slod_amd.C.byref(out)) == -1 and not out.value
    assert lib.slod_last_error(other.h).decode() == "slod_lod_sources_create: receivers of another handle"
    assert lib.slod_lod_inject_multi(other.h, S1.s, G.data_ptr(), K, K, None, 0, B.data_ptr(), K, None) == -1
    assert lib.slod_last_error(other.h).decode() == "slod_lod_inject_multi: sources of another handle"
    assert lib.slod_lod_inject_ensemble(other.h, SK.s, 0, K, G.data_ptr(), K, None, 0, B.data_ptr(), K, None) == -1
    assert lib.slod_last_error(other.h).decode() == "slod_lod_inject_ensemble: sources of another handle"
    refused(lambda: SK.inject(G.data_ptr(), B.data_ptr(), n_rhs=K), "slod_lod_inject_multi: sources of another member count")
    refused(lambda: SK.inject_ensemble(G.data_ptr(), B.data_ptr(), n_members=K, first_member=1), "members outside the sources")
    refused(lambda: SK.inject_ensemble(G.data_ptr(), B.data_ptr(), n_members=1, first_member=-1), "members outside the sources")
    refused(lambda: S1.inject_ensemble(G.data_ptr(), B.data_ptr(), n_members=2), "members outside the sources")
    refused(lambda: S1.inject(G.data_ptr(), B.data_ptr(), n_rhs=0), "slod_lod_inject_multi: n_rhs < 1")
    refused(lambda: SK.inject_ensemble(G.data_ptr(), B.data_ptr(), n_members=0), "slod_lod_inject_ensemble: n_members < 1")
    refused(lambda: S1.inject(G.data_ptr(), B.data_ptr(), n_rhs=3, ld_g=2), "leading dimension below n_rhs")
    refused(lambda: S1.inject(G.data_ptr(), B.data_ptr(), n_rhs=3, ld_b=2), "leading dimension below n_rhs")
    refused(lambda: S1.inject(G.data_ptr(), B.data_ptr(), n_rhs=3, d_base=B.data_ptr(), ld_base=2), "leading dimension below n_rhs")
    refused(lambda: SK.inject_ensemble(G.data_ptr(), B.data_ptr(), ld_g=2), "leading dimension below n_members")
    refused(lambda: S1.inject(0, B.data_ptr()), "NULL sources or array")
    refused(lambda: S1.inject(G.data_ptr(), 0), "NULL sources or array")
    _sync()
    assert (_bits(B) == SENT_BITS).all()                                  # no refused call wrote
    S1.inject(G.data_ptr(), B.data_ptr(), n_rhs=3, ld_base=0)             # without a base its ld is not looked at
    _sync()
    assert (_bits(B) != SENT_BITS).all()
    for o in (R1, RK, S1, SK):
        o.close()
    other.close()
