"""GPU tests of the record of the time loops on the LOD space (slod_lod_time_record_arm) on real pencils
(lod_cases._pencil: step64, s2, rowmajor) and on the ensemble configurations of lod_irk_ensemble_cases (members const /
D100 / D1e4), six receivers each: a coarse-cell corner, a cell-interior node, a node next to the boundary, a boundary
node, a 4-term point and a 2-term difference.

For each of the ten steppers, n_steps = 7, every 1 and 3, what U, V and U|V where the loop has a v: the armed call leaves
the words of the un-armed call in every output; record j has the words of slod_lod_observe_* of the state a separate
un-armed call with n_steps = j every leaves; every other word of d_trace keeps its sentinel.  Then the one-shot rule,
every record refusal by message, the ensemble trace against the single stepper per member (K = 3 and K = 65), the trace
against O_dense u_k of dense numpy recursions within lod_irk_cases.FORWARD = 1e-8 max |reference|, and two physical runs.

Measured on an MI355X (printed by the tests; DESIGN section 6, "Receivers"): worst |trace - O_dense u_k| / max |reference|
of test_trace_against_the_dense_recursion 5.7e-15 (theta CG 5.4e-15, theta factor 3.0e-16, Newmark CG 3.3e-15, Newmark
factor 1.8e-15, Radau heat 3.2e-16, Gauss wave 5.7e-15) against the bar 1e-8.  The eigenmode trace reaches 1.000 of the
scheme's own bound |R^k - e^{ik theta}| amp (the bound is attained where k theta is near pi / 2: the error is its real part,
|sin k theta| of it, 0.9998 at k = 31), with a rounding term of 1.2e-12 amp at k = 40 (cond(S) = 41).  The backward Euler
trace stays within 0.18 of its derived bound and ends at 2.6e-8 of the first distance."""
import os
import re
import subprocess

import numpy as np
import pytest

import lod_irk_cases as ic
import lod_irk_ensemble_cases as ec
from lod_cases import _bits, _pencil, _torch

pytestmark = pytest.mark.gpu

N_STEPS = 7
SENT_BITS = 0x5a5a5a5a5a5a5a5a
SENT = np.array([SENT_BITS], dtype=np.uint64).view(np.float64)[0]
SINGLE = ("theta_cg", "theta_direct", "nm_cg", "nm_direct", "irk_heat", "irk_wave")
ENSEMBLE = ("theta_ens", "nm_ens", "irk_heat_ens", "irk_wave_ens")
U, V = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")


def _sync():
    _torch()[0].cuda.synchronize()


def _sent(*shape):
    torch, dev = _torch()
    return torch.full(shape, float(SENT), dtype=torch.float64, device=dev)


def _six(g, s):
    """The six receivers of a handle."""
    import slod_amd
    n, N, NE = g.cfg.n_subdivisions, g.N, g.NE
    NEp = NE + 1
    corner = n * (N // 2) + n * (N // 2) * NEp
    interior = (n + 1) + (2 * n + 1) * NEp
    near = 1 + (NE // 2) * NEp
    boundary = 0 + (NE // 2) * NEp
    return [[(corner, 0, 1.0)], [(interior, s - 1, 1.0)], [(near, 0, 1.0)], [(boundary, s - 1, 1.0)],
            slod_amd.point_terms(NE, s, 0.43, 0.58, s - 1), [(corner, 0, 1.0), (interior, s - 1, -1.0)]]


class _Stepper:
    """One of the ten steppers on fixed matrices and a fixed factor: run(state, n_steps) advances state (a dict of device
    tensors u, v, a with padded leading dimensions) in place and returns the host outputs of the call."""

    def __init__(self, name, g, ncol, has_v, ens, run, recv, keep):
        self.name, self.g, self.ncol, self.has_v, self.ens, self.run, self.recv, self.keep = name, g, ncol, has_v, ens, run, recv, keep

    def observe(self, x):
        torch, dev = _torch()
        y = _sent(self.recv.n_recv, self.ncol)
        if self.ens:
            self.recv.observe_ensemble(x.data_ptr(), y.data_ptr(), n_members=self.ncol, ld_u=x.shape[1])
        else:
            self.recv.observe(x.data_ptr(), y.data_ptr(), n_rhs=self.ncol, ld_u=x.shape[1])
        _sync()
        return _bits(y)


_steppers = {}


def _state(nrow, ncol, seed, scale_v):
    rng = np.random.default_rng(seed)
    return {"u": ec.padded(rng.uniform(-1.0, 1.0, (nrow, ncol)), 1), "v": ec.padded(rng.uniform(-1.0, 1.0, (nrow, ncol)) * scale_v, 2),
            "a": ec.nan(nrow, ncol + 1)}


def _single(so, kind, name="step64", ncol=2):
    key = (kind, name, ncol)
    if key in _steppers:
        return _steppers[key]
    c = _pencil(so, name)
    g, cols, A, M = c.g, c.cols.data_ptr(), c.sym.data_ptr(), c.mvalues.data_ptr()
    lam = c.lam
    recv = g.lod_receivers(_six(g, c.s), c.b.data_ptr(), c.stride)
    w1 = np.sqrt(lam[0])
    st0 = _state(c.nrow, ncol, 11, w1)
    keep = []

    def comb(alpha, beta):
        S = ec.nan(c.sym.numel())
        g.lod_matrix_combine(alpha, M, beta, A, S.data_ptr())
        keep.append(S)
        return g.lod_factor(S.data_ptr(), cols)

    lds = lambda s: dict(ld_u=s["u"].shape[1], ld_v=s["v"].shape[1], ld_a=s["a"].shape[1])
    if kind in ("nm_cg", "nm_direct"):
        g.lod_newmark_accel(A, M, cols, st0["u"].data_ptr(), st0["v"].data_ptr(), st0["a"].data_ptr(), n_rhs=ncol, **lds(st0))
    if kind == "theta_cg":
        dt = 0.1 / lam[0]
        run = lambda s, k: g.lod_theta_steps(A, M, cols, dt, 0.5, k, s["u"].data_ptr(), n_rhs=ncol, ld_u=s["u"].shape[1])
    elif kind == "theta_direct":
        dt = 0.1 / lam[0]
        f = comb(1.0, 0.5 * dt)
        run = lambda s, k: g.lod_theta_steps_direct(f, A, cols, dt, 0.5, k, s["u"].data_ptr(), n_rhs=ncol, ld_u=s["u"].shape[1])
    elif kind == "nm_cg":
        dt = 0.5 / w1
        run = lambda s, k: g.lod_newmark_steps(A, M, cols, dt, k, s["u"].data_ptr(), s["v"].data_ptr(), s["a"].data_ptr(), n_rhs=ncol,
                                               **lds(s))
    elif kind == "nm_direct":
        dt = 0.5 / w1
        f = comb(1.0, 0.25 * dt * dt)
        run = lambda s, k: g.lod_newmark_steps_direct(f, A, M, cols, dt, k, s["u"].data_ptr(), s["v"].data_ptr(), s["a"].data_ptr(),
                                                      n_rhs=ncol, **lds(s))
    elif kind == "irk_heat":
        dt = 0.1 / lam[0]
        f = g.lod_factor_zldl(A, M, cols, *[[x] for x in g.lod_irk_coefficients("radau", 1, dt)])
        run = lambda s, k: g.lod_irk_heat_steps(f, "radau", A, cols, dt, k, s["u"].data_ptr(), n_rhs=ncol, ld_u=s["u"].shape[1])
    else:
        dt = 0.5 / w1
        f = g.lod_factor_zldl(A, M, cols, *[[x] for x in g.lod_irk_coefficients("gauss", 2, dt)])
        run = lambda s, k: g.lod_irk_wave_steps(f, "gauss", A, M, cols, dt, k, s["u"].data_ptr(), s["v"].data_ptr(), n_rhs=ncol,
                                                ld_u=s["u"].shape[1], ld_v=s["v"].shape[1])
    st = _Stepper(kind, g, ncol, kind in ("nm_cg", "nm_direct", "irk_wave"), False, run, recv, keep)
    st.state0, st.dt, st.c = st0, dt, c
    _steppers[key] = st
    return st


def _ens_slab(c, K):
    """The basis slabs of the K members of lod_irk_ensemble_cases.stack: the three members, then copies (a scaled matrix
    pair has its member's basis)."""
    torch, dev = _torch()
    return c.b if K == c.K else torch.cat([c.slab[k % c.K][0] for k in range(K)])


def _ensemble(so, kind, name="base", K=3):
    key = (kind, name, K)
    if key in _steppers:
        return _steppers[key]
    c = ec.ens_case(so, name)
    g, cols = c.g, c.cols.data_ptr()
    At, Mt = ec.stack(c, c.sym, K, 1), ec.stack(c, c.mass, K, 2)
    A, M, lda, ldm = At.data_ptr(), Mt.data_ptr(), K + 1, K + 2
    lam1, lamn = ec.joint_spectrum(c.lam)
    slab = _ens_slab(c, K)
    recv = g.lod_receivers(_six(g, c.s), slab.data_ptr(), c.stride, n_members=K, member_stride=c.mstride)
    w1 = np.sqrt(lam1)
    st0 = _state(c.nrow, K, 12, w1)
    keep = [At, Mt, slab]
    lds = lambda s: dict(ld_u=s["u"].shape[1], ld_v=s["v"].shape[1], ld_a=s["a"].shape[1])

    def comb(alpha, beta):
        S = ec.nan(c.nval, K)
        g.lod_matrix_combine_ensemble(alpha, M, beta, A, K, S.data_ptr(), ld_a=ldm, ld_b=lda)
        keep.append(S)
        return g.lod_factor_ensemble(S.data_ptr(), cols, K)

    if kind == "theta_ens":
        dt = 0.1 / lam1
        f = comb(1.0, 0.5 * dt)
        run = lambda s, k: g.lod_theta_steps_ensemble_direct(f, A, cols, dt, 0.5, k, K, s["u"].data_ptr(), ld_m=lda, ld_u=s["u"].shape[1])
    elif kind == "nm_ens":
        dt = 0.5 / w1
        fM = comb(1.0, 0.0)
        g.lod_newmark_accel_ensemble_direct(fM, A, M, cols, K, st0["u"].data_ptr(), st0["v"].data_ptr(), st0["a"].data_ptr(), ld_a_m=lda,
                                            ld_m_m=ldm, **lds(st0))
        _sync()
        f = comb(1.0, 0.25 * dt * dt)
        run = lambda s, k: g.lod_newmark_steps_ensemble_direct(f, A, M, cols, dt, k, K, s["u"].data_ptr(), s["v"].data_ptr(),
                                                               s["a"].data_ptr(), ld_a_m=lda, ld_m_m=ldm, **lds(s))
    elif kind == "irk_heat_ens":
        dt = 0.1 / lam1
        a, b = g.lod_irk_coefficients("radau", 1, dt)
        f = g.lod_factor_zldl_ensemble(A, M, cols, K, [a], [b], ld_a_m=lda, ld_b_m=ldm)
        run = lambda s, k: g.lod_irk_heat_steps_ensemble(f, "radau", A, cols, dt, k, K, s["u"].data_ptr(), ld_a_m=lda, ld_u=s["u"].shape[1])
    else:
        dt = 0.5 / w1
        a, b = g.lod_irk_coefficients("gauss", 2, dt)
        f = g.lod_factor_zldl_ensemble(A, M, cols, K, [a], [b], ld_a_m=lda, ld_b_m=ldm)
        run = lambda s, k: g.lod_irk_wave_steps_ensemble(f, "gauss", A, M, cols, dt, k, K, s["u"].data_ptr(), s["v"].data_ptr(),
                                                         ld_a_m=lda, ld_m_m=ldm, ld_u=s["u"].shape[1], ld_v=s["v"].shape[1])
    st = _Stepper(kind, g, K, kind in ("nm_ens", "irk_wave_ens"), True, run, recv, keep)
    st.state0, st.dt, st.c = st0, dt, c
    _steppers[key] = st
    return st


def _get(so, kind, **kw):
    return _single(so, kind, **kw) if kind in SINGLE else _ensemble(so, kind, **kw)


def _clone(state):
    return {k: t.clone() for k, t in state.items()}


def _host(extra):
    """The host outputs of a stepper call as a tuple of arrays of words."""
    if extra is None:
        return ()
    out = []
    for a in (extra if isinstance(extra, tuple) else (extra,)):
        if a is not None:
            a = np.ascontiguousarray(a)
            out.append(a.view(np.uint64) if a.dtype == np.float64 else a.copy())
    return tuple(out)


def _run(st, n_steps, arm=None):
    """A call from the entry state; arm() is called right before it.  Returns (state words, host outputs)."""
    s = _clone(st.state0)
    if arm is not None:
        arm()
    extra = st.run(s, n_steps)
    _sync()
    return {k: _bits(t) for k, t in s.items()}, _host(extra), s


def _same_outputs(a, b):
    return all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


class _Trace:
    """A sentinel-filled trace buffer with padding in ld_trace, between records and a spare record at the end."""

    def __init__(self, st, what, every, n_steps=N_STEPS):
        self.st, self.what, self.every = st, what, every
        self.nq = 2 if what == (U | V) else 1
        self.nrec = n_steps // every + 1
        self.ld = st.ncol + 1
        self.stride = self.nq * st.recv.n_recv * self.ld + 3
        self.t = _sent((self.nrec + 1) * self.stride)

    def arm(self, **kw):
        a = dict(capacity=self.nrec, what=self.what, every=self.every, ld_trace=self.ld, record_stride=self.stride)
        a.update(kw)
        return self.st.g.lod_time_record(self.st.recv, self.t.data_ptr(), **a)

    def expected(self, records):
        """records[j] = list of nq arrays [n_recv][ncol] of words"""
        want = np.full((self.nrec + 1) * self.stride, SENT_BITS, dtype=np.uint64)
        nr, nc = self.st.recv.n_recv, self.st.ncol
        for j, quantities in enumerate(records):
            for w, y in enumerate(quantities):
                blk = want[j * self.stride + w * nr * self.ld:j * self.stride + (w + 1) * nr * self.ld].reshape(nr, self.ld)
                blk[:, :nc] = y
        return want

    def untouched(self):
        return bool((_bits(self.t) == SENT_BITS).all())


_refs = {}


def _reference_records(so, kind, every, **kw):
    """Per record j the words of observe(u), observe(v) of the state an un-armed call with n_steps = j every leaves."""
    key = (kind, every, tuple(sorted(kw.items())))
    if key not in _refs:
        st = _get(so, kind, **kw)
        out = []
        for j in range(N_STEPS // every + 1):
            s = _clone(st.state0)
            if j:
                st.run(s, j * every)
                _sync()
            out.append((st.observe(s["u"]), st.observe(s["v"]) if st.has_v else None))
        _refs[key] = out
    return _refs[key]


CASES = [(kind, name) for kind in SINGLE for name in ("step64", "s2", "rowmajor")] + [(kind, name) for kind in ENSEMBLE for name in ec.NAMES]


@pytest.mark.parametrize("kind,name", CASES)
def test_record_and_no_perturbation(so, kind, name):
    st = _get(so, kind, name=name)
    base = _run(st, N_STEPS)
    for every in (1, 3):
        ref = _reference_records(so, kind, every, name=name)
        for what in ((U, V, U | V) if st.has_v else (U,)):
            tr = _Trace(st, what, every)
            armed = _run(st, N_STEPS, tr.arm)
            assert _same_outputs(base, armed), (kind, every, what)
            pick = {U: lambda r: [r[0]], V: lambda r: [r[1]], U | V: lambda r: [r[0], r[1]]}[what]
            want = tr.expected([pick(r) for r in ref])
            assert len(ref) == tr.nrec == N_STEPS // every + 1
            assert np.array_equal(_bits(tr.t), want), (kind, every, what)
            assert np.isfinite(_bits(tr.t)[_bits(tr.t) != SENT_BITS].view(np.float64)).all()
    # record 0 is the entry state, and with every = 3 the state after step 7 is not in the trace
    ref1, ref3 = _reference_records(so, kind, 1, name=name), _reference_records(so, kind, 3, name=name)
    assert np.array_equal(ref1[0][0], st.observe(st.state0["u"])) and np.array_equal(ref3[2][0], ref1[6][0])
    assert not any(np.array_equal(r[0], ref1[7][0]) for r in ref3)


@pytest.mark.parametrize("kind", SINGLE + ENSEMBLE)
def test_one_shot(so, kind):
    import slod_amd
    st = _get(so, kind)
    base = _run(st, N_STEPS)
    tr = _Trace(st, U, 1)
    # the same stepper again right after an armed call, un-armed by the caller: nothing is recorded
    _run(st, N_STEPS, tr.arm)
    assert not tr.untouched()
    tr.t.fill_(float(SENT))
    again = _run(st, N_STEPS)
    assert tr.untouched() and _same_outputs(base, again)
    # a call refused by one of its own checks consumes the arming
    tr.arm()
    with pytest.raises(slod_amd.SlodError) as e:
        st.run(_clone(st.state0), 0)
    assert e.value.code == -1 and "n_steps < 1" in str(e.value)
    _run(st, N_STEPS)
    assert tr.untouched()
    # so does a record refusal
    tr.arm(every=0)
    with pytest.raises(slod_amd.SlodError) as e:
        st.run(_clone(st.state0), N_STEPS)
    assert "record: every < 1" in str(e.value)
    _run(st, N_STEPS)
    assert tr.untouched()
    # disarming by hand
    tr.arm()
    st.g.lod_time_record(None, 0)
    _run(st, N_STEPS)
    assert tr.untouched()
    # destroying the receivers a record names disarms it: the next call runs as an un-armed one
    c = st.c
    gone = st.g.lod_receivers(_six(st.g, c.s), c.b.data_ptr(), c.stride, n_members=st.ncol if st.ens else 1,
                              member_stride=c.mstride if st.ens and st.ncol == c.K else 0)
    st.g.lod_time_record(gone, tr.t.data_ptr(), capacity=tr.nrec, ld_trace=tr.ld, record_stride=tr.stride)
    gone.close()
    assert _same_outputs(base, _run(st, N_STEPS)) and tr.untouched()


def test_other_calls_do_not_consume_the_arming(so):
    st = _single(so, "nm_direct")
    c, g = st.c, st.g
    want = _Trace(st, U | V, 1)
    _run(st, N_STEPS, want.arm)
    tr = _Trace(st, U | V, 1)
    tr.arm()
    fM = g.lod_factor(c.mvalues.data_ptr(), c.cols.data_ptr())
    s = _clone(st.state0)
    acc, y = ec.nan(c.nrow, st.ncol + 1), ec.nan(c.nrow, st.ncol)
    g.lod_newmark_accel_direct(fM, c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), s["u"].data_ptr(), s["v"].data_ptr(),
                               acc.data_ptr(), n_rhs=st.ncol, ld_u=s["u"].shape[1], ld_v=s["v"].shape[1], ld_a=acc.shape[1])
    g.lod_apply(c.sym.data_ptr(), c.cols.data_ptr(), s["u"].data_ptr(), y.data_ptr(), n_rhs=st.ncol, ld_x=s["u"].shape[1])
    st.observe(s["u"])
    _sync()
    assert tr.untouched()
    st.run(s, N_STEPS)
    _sync()
    assert np.array_equal(_bits(tr.t), _bits(want.t))
    fM.close()


@pytest.mark.parametrize("kind", SINGLE + ENSEMBLE)
def test_record_refusals(so, kind):
    import slod_amd
    st = _get(so, kind)
    tr = _Trace(st, U, 1)
    nr, nc = st.recv.n_recv, st.ncol
    other = _single(so, "theta_direct", name="rowmajor").recv                    # a handle of its own
    c = st.c
    if st.ens:
        wrong_members = st.g.lod_receivers(_six(st.g, c.s), c.b.data_ptr(), c.stride)
    else:
        wrong_members = st.g.lod_receivers(_six(st.g, c.s), c.b.data_ptr(), c.stride, n_members=2, member_stride=0)
    cases = [(dict(what=0), "record: what is SLOD_RECORD_U, SLOD_RECORD_V or both"),
             (dict(what=4), "record: what is SLOD_RECORD_U, SLOD_RECORD_V or both"),
             (dict(every=0), "record: every < 1"), (dict(every=-3), "record: every < 1"),
             (dict(ld_trace=nc - 1), "record: ld_trace below " + ("n_members" if st.ens else "n_rhs")),
             (dict(record_stride=nr * tr.ld - 1), "record: record_stride below n_quantities n_recv ld_trace"),
             (dict(capacity=N_STEPS), "record: capacity below n_steps / every + 1"),          # one too few
             (dict(capacity=2, every=3), "record: capacity below n_steps / every + 1")]
    if st.has_v:
        cases.append((dict(what=U | V, record_stride=2 * nr * tr.ld - 1), "record: record_stride below n_quantities n_recv ld_trace"))
    else:
        cases += [(dict(what=V), "record: SLOD_RECORD_V in a loop without a velocity"),
                  (dict(what=U | V), "record: SLOD_RECORD_V in a loop without a velocity")]
    for kw, word in cases:
        tr.arm(**kw)
        with pytest.raises(slod_amd.SlodError) as e:
            st.run(_clone(st.state0), N_STEPS)
        assert e.value.code == -1 and word in str(e.value) and str(e.value).count("slod_lod_") >= 1, (kw, str(e.value))
    # a NULL d_trace, the receivers of another handle, another member count
    for recv, ptr, word in ((st.recv, 0, "record: NULL d_trace"), (other, tr.t.data_ptr(), "record: receivers of another handle"),
                            (wrong_members, tr.t.data_ptr(), "record: receivers of another member count")):
        st.g.lod_time_record(recv, ptr, capacity=tr.nrec, ld_trace=tr.ld, record_stride=tr.stride)
        with pytest.raises(slod_amd.SlodError) as e:
            st.run(_clone(st.state0), N_STEPS)
        assert e.value.code == -1 and word in str(e.value), str(e.value)
    _sync()
    assert tr.untouched()
    # the stepper's own checks come first
    tr.arm(every=0)
    with pytest.raises(slod_amd.SlodError) as e:
        st.run(_clone(st.state0), -1)
    assert "record" not in str(e.value)
    # exactly enough is taken
    tr.arm(capacity=N_STEPS + 1)
    st.run(_clone(st.state0), N_STEPS)
    _sync()
    assert not tr.untouched()
    wrong_members.close()


def _member_single(so, ens, k):
    """The single stepper of member k of an ensemble stepper: de-interleaved matrices, a one-member factor, a one-member
    receivers object on member k's slab; the state is column k."""
    c, g, K, kind, dt = ens.c, ens.g, ens.ncol, ens.name, ens.dt
    f = ec.scale(K, k, c.K)
    Ak, Mk = (c.sym[k % c.K] * f).contiguous(), (c.mass[k % c.K] * f).contiguous()
    A, M, cols = Ak.data_ptr(), Mk.data_ptr(), c.cols.data_ptr()
    recv = g.lod_receivers(_six(g, c.s), c.slab[k % c.K][0].data_ptr(), c.stride)
    s = {n: t[:, k:k + 1].contiguous() for n, t in ens.state0.items()}
    trace = _sent(N_STEPS + 1, 2 if ens.has_v else 1, recv.n_recv)
    g.lod_time_record(recv, trace.data_ptr(), capacity=N_STEPS + 1, what=U | V if ens.has_v else U)

    def comb(alpha, beta):
        S = ec.nan(c.nval)
        g.lod_matrix_combine(alpha, M, beta, A, S.data_ptr())
        return g.lod_factor(S.data_ptr(), cols), S

    if kind == "theta_ens":
        fk, S = comb(1.0, 0.5 * dt)
        g.lod_theta_steps_direct(fk, A, cols, dt, 0.5, N_STEPS, s["u"].data_ptr())
    elif kind == "nm_ens":
        fk, S = comb(1.0, 0.25 * dt * dt)
        g.lod_newmark_steps_direct(fk, A, M, cols, dt, N_STEPS, s["u"].data_ptr(), s["v"].data_ptr(), s["a"].data_ptr())
    elif kind == "irk_heat_ens":
        fk = g.lod_factor_zldl(A, M, cols, *[[x] for x in g.lod_irk_coefficients("radau", 1, dt)])
        g.lod_irk_heat_steps(fk, "radau", A, cols, dt, N_STEPS, s["u"].data_ptr())
    else:
        fk = g.lod_factor_zldl(A, M, cols, *[[x] for x in g.lod_irk_coefficients("gauss", 2, dt)])
        g.lod_irk_wave_steps(fk, "gauss", A, M, cols, dt, N_STEPS, s["u"].data_ptr(), s["v"].data_ptr())
    _sync()
    fk.close(), recv.close()
    return _bits(trace)


@pytest.mark.parametrize("K", (3, 65))
@pytest.mark.parametrize("kind", ENSEMBLE)
def test_ensemble_trace_equals_the_single_stepper_per_member(so, kind, K):
    st = _ensemble(so, kind, K=K)
    nq, nr = 2 if st.has_v else 1, st.recv.n_recv
    trace = _sent(N_STEPS + 1, nq, nr, K)
    st.g.lod_time_record(st.recv, trace.data_ptr(), capacity=N_STEPS + 1, what=U | V if st.has_v else U, columns=K)
    st.run(_clone(st.state0), N_STEPS)
    _sync()
    got = _bits(trace)
    assert (got != SENT_BITS).all()
    for k in range(K):
        assert np.array_equal(got[..., k], _member_single(so, st, k)), (kind, K, k)


def _dense_rows(recv, nrow, member=0):
    rb, cols, vals = recv.rows(member)
    O = np.zeros((recv.n_recv, nrow))
    for q in range(recv.n_recv):
        np.add.at(O[q], cols[rb[q]:rb[q + 1]], vals[rb[q]:rb[q + 1]])
    return O


def _dense_states(kind, A, M, dt, u, v, a):
    """[n_steps + 1] states (u, v) of the dense recursion of a scheme: theta = 1/2, the trapezoidal rule in acceleration
    form, or the undiagonalised stage system of lod_irk_cases."""
    if kind.startswith("theta"):
        S, us = M + 0.5 * dt * A, [u]
        for _ in range(N_STEPS):
            u = u + np.linalg.solve(S, dt * (-(A @ u)))
            us.append(u)
        return np.array(us), None
    if kind.startswith("nm"):
        S, us, vs = M + 0.25 * dt * dt * A, [u], [v]
        for _ in range(N_STEPS):
            ut, vt = u + dt * v + 0.25 * dt * dt * a, v + 0.5 * dt * a
            a = np.linalg.solve(S, -(A @ ut))
            u, v = ut + 0.25 * dt * dt * a, vt + 0.5 * dt * a
            us.append(u), vs.append(v)
        return np.array(us), np.array(vs)
    if kind == "irk_heat":
        return ic.heat_stage(A, M, ic.RADAU, dt, N_STEPS, u), None
    return ic.wave_stage(A, M, ic.GAUSS, dt, N_STEPS, u, v)


@pytest.mark.parametrize("kind", SINGLE)
def test_trace_against_the_dense_recursion(so, kind):
    """One CG, one factor and one IRK loop per equation: the trace against O_dense u_k (and v_k) of the dense recursion
    within lod_irk_cases.FORWARD = 1e-8 of max |reference|."""
    st = _single(so, kind)
    c = st.c
    what = U | V if st.has_v else U
    nq, nr = (2 if st.has_v else 1), st.recv.n_recv
    trace = _sent(N_STEPS + 1, nq, nr, st.ncol)
    st.g.lod_time_record(st.recv, trace.data_ptr(), capacity=N_STEPS + 1, what=what, columns=st.ncol)
    st.run(_clone(st.state0), N_STEPS)
    _sync()
    got = trace.cpu().numpy()
    O = _dense_rows(st.recv, c.nrow)
    h = {k: t[:, :st.ncol].cpu().numpy() for k, t in st.state0.items()}
    us, vs = _dense_states(kind, c.A, c.M, st.dt, h["u"], h["v"], h["a"])
    worst = 0.0
    for w, xs in enumerate((us, vs)[:nq]):
        ref = np.einsum("qr,krc->kqc", O, xs)
        err = np.abs(got[:, w] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
    print("trace against the dense recursion, %s: worst |trace - O u_k| / max |reference| = %.3e" % (kind, worst))
    assert worst <= ic.FORWARD, (kind, worst)


def test_backward_euler_trace_converges_to_the_elliptic_value(so):
    """Backward Euler with a constant load: the trace at an interior node tends to the nodal value of the reconstructed
    elliptic solution, and the distance does not increase."""
    torch, dev = _torch()
    c = _pencil(so, "step64")
    g, cols, A, M = c.g, c.cols.data_ptr(), c.sym.data_ptr(), c.mvalues.data_ptr()
    fine = torch.zeros((g.NE + 1) ** 2 * c.s, dtype=torch.float64, device=dev)
    g.fem_rhs(None, fine.data_ptr())
    b = ec.nan(c.nrow)
    g.lod_rhs(c.ids, c.b.data_ptr(), c.stride, fine.data_ptr(), b.data_ptr())
    fA = g.lod_factor(A, cols)
    u_inf = ec.nan(c.nrow)
    fA.solve(b.data_ptr(), u_inf.data_ptr())
    node = (g.NE // 2 + 1) + (g.NE // 2 + 1) * (g.NE + 1)
    recv = g.lod_receivers([[(node, 0, 1.0)]], c.b.data_ptr(), c.stride)
    full = ec.nan((g.NE + 1) ** 2 * c.s)
    g.lod_reconstruct(c.b.data_ptr(), c.stride, u_inf.data_ptr(), full.data_ptr())
    _sync()
    target = float(full[node * c.s])
    dt, steps = 2.0 / c.lam[0], 16
    S = ec.nan(c.sym.numel())
    g.lod_matrix_combine(1.0, M, dt, A, S.data_ptr())
    f = g.lod_factor(S.data_ptr(), cols)
    u = torch.zeros(c.nrow, dtype=torch.float64, device=dev)
    trace = _sent(steps + 1)
    g.lod_time_record(recv, trace.data_ptr(), capacity=steps + 1)
    g.lod_theta_steps_direct(f, A, cols, dt, 1.0, steps, u.data_ptr(), d_load=b.data_ptr())
    _sync()
    dist = np.abs(trace.cpu().numpy() - target)
    assert dist[0] == abs(target) > 0.0
    assert (np.diff(dist) <= 0.0).all(), dist
    # Convergence, derived: e_k = u_k - u_inf = (I + dt M^-1 A)^-k e_0 shrinks in the M-norm by 1 / (1 + dt lam_1) = 1/3 a
    # step, and |O e| <= sqrt(O M^-1 O^T) ||e||_M for the row O of the receiver, so
    #   dist_k <= 3^-k sqrt(O M^-1 O^T) sqrt(u_inf^T M u_inf),
    # plus the rounding of k solves and of the two products, (k + 2) 2^-53 cond(S) ||O|| ||u_inf|| with cond(S) <= lam_n / lam_1.
    O = _dense_rows(recv, c.nrow)[0]
    ui = u_inf.cpu().numpy()
    k = np.arange(steps + 1)
    bound = 3.0 ** -k * np.sqrt(O @ np.linalg.solve(c.M, O)) * np.sqrt(ui @ c.M @ ui)
    bound = bound + (k + 2) * 2.0 ** -53 * (c.lam[-1] / c.lam[0]) * np.linalg.norm(O) * np.linalg.norm(ui)
    print("backward Euler trace: worst distance / bound = %.3f, last distance / first = %.3e" % ((dist / bound).max(), dist[-1] / dist[0]))
    assert (dist <= bound).all(), (dist / bound).max()
    for o in (fA, f, recv):
        o.close()


def test_gauss_wave_trace_follows_the_eigenmode(so):
    """The undamped wave started in the generalised eigenvector j with Gauss IRK at dt = 0.05 / sqrt(lam_j): the trace
    follows cos(sqrt(lam_j) t_k) (C x_j)(node).  The bar is the scheme's own global error on that mode: the Pade stability
    function against e^{i theta}, |R(i theta)^k - e^{i k theta}| (|R| = 1 for Gauss), times the mode's amplitude at the node.
    It is 0 at k = 0 while the fma chain and the numpy product round differently, so a derived rounding term is added:
    ((k + 1) cond(S) + m) 2^-53 ||O|| ||x_j||, one solve with the step matrix S = M + z^2 A per step (cond from the dense
    pencil) and the m products of the receiver's row O; about 1e-13 of the amplitude, four orders below the scheme's bound
    after one step (4.3e-10)."""
    torch, dev = _torch()
    c = _pencil(so, "step64")
    g, cols, A, M = c.g, c.cols.data_ptr(), c.sym.data_ptr(), c.mvalues.data_ptr()
    j, steps = 1, 40
    lam, x = c.lam[j], c.vec[:, j]
    w = np.sqrt(lam)
    dt = 0.05 / w
    node = (g.NE // 4 + 1) + (g.NE // 4) * (g.NE + 1)          # off the nodal lines of the lowest modes of the square
    recv = g.lod_receivers([[(node, 0, 1.0)]], c.b.data_ptr(), c.stride)
    amp = float((_dense_rows(recv, c.nrow) @ x)[0])
    f = g.lod_factor_zldl(A, M, cols, *[[t] for t in g.lod_irk_coefficients("gauss", 2, dt)])
    u, v = ec.dev(x.reshape(-1, 1)), torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev)
    trace = _sent(steps + 1)
    g.lod_time_record(recv, trace.data_ptr(), capacity=steps + 1)
    g.lod_irk_wave_steps(f, "gauss", A, M, cols, dt, steps, u.data_ptr(), v.data_ptr(), energies=False)
    _sync()
    k = np.arange(steps + 1)
    theta = w * dt
    R = ic.stability(ic.GAUSS, 1j * theta)
    assert abs(abs(R) - 1.0) <= 1e-15
    scheme = np.abs(R ** k - np.exp(1j * k * theta)) * abs(amp)
    O = _dense_rows(recv, c.nrow)[0]
    z = dt * ic.LAMBDA[ic.GAUSS]
    cond = np.linalg.cond(c.M + z * z * c.A)
    rounding = ((k + 1) * cond + np.count_nonzero(O)) * 2.0 ** -53 * np.linalg.norm(O) * np.linalg.norm(x)
    bound = scheme + rounding
    err = np.abs(trace.cpu().numpy() - np.cos(w * dt * k) * amp)
    print("eigenmode trace: worst error / scheme's bound (k >= 1) = %.3f, worst error / (scheme's bound + rounding) = %.3f, "
          "rounding term / amplitude at k = %d: %.3e, cond(S) = %.3e, amplitude %.3e"
          % ((err[1:] / scheme[1:]).max(), (err / bound).max(), steps, rounding[-1] / abs(amp), cond, amp))
    assert abs(amp) > 0.0 and (err <= bound).all(), (err / bound).max()
    f.close(), recv.close()


def test_pipeline_plan_to_trace(so):
    """plan -> matrices -> factor -> receivers -> 4 armed steps -> trace, on a fresh handle."""
    import slod_amd
    from lod_cases import _build, _mass, _symmetrize
    torch, dev = _torch()
    c = _build(so, dict(nref=2, n_sub=2, oversampling=1, spacedim=1))
    g = c.g
    c.mvalues, _ = _mass(c)
    sym = _symmetrize(c)
    dt = 1e-3
    S = ec.nan(sym.numel())
    g.lod_matrix_combine(1.0, c.mvalues.data_ptr(), dt, sym.data_ptr(), S.data_ptr())
    f = g.lod_factor(S.data_ptr(), c.cols.data_ptr())
    recv = g.lod_receivers([slod_amd.point_terms(g.NE, 1, 0.5, 0.5), [(g.NE + 2, 0, 1.0)]], c.b.data_ptr(), c.stride)
    u = ec.dev(np.random.default_rng(3).uniform(0.0, 1.0, (c.nrow, 1)))
    u0 = u.clone()
    trace = _sent(5, 2)
    g.lod_time_record(recv, trace.data_ptr(), capacity=5)
    g.lod_theta_steps_direct(f, sym.data_ptr(), c.cols.data_ptr(), dt, 1.0, 4, u.data_ptr())
    _sync()
    t = trace.cpu().numpy()
    y0, y4 = _sent(2, 1), _sent(2, 1)
    recv.observe(u0.data_ptr(), y0.data_ptr())
    recv.observe(u.data_ptr(), y4.data_ptr())
    _sync()
    assert np.isfinite(t).all() and np.array_equal(t[0].view(np.uint64), _bits(y0).ravel()) and np.array_equal(t[4].view(np.uint64), _bits(y4).ravel())
    g.close()


def _driver(*args):
    """A fresh child process per run, under its own time limit."""
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "2", "1", "1", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


TRACE_LINE = r"^wave receiver (\d+) member (\d+) record (\d+): t = (\S+), u = (\S+), v = (\S+)$"


def test_driver_receiver_lines():
    """main_Diffusion 3 2 1 1 --ensemble 3 --wave 4 DT --direct --receiver .. --receiver .. --record-every 2: one line per
    record, receiver and member, (n_steps / every + 1) * receivers * members in all, and the lines of member m are those of
    a --member m run, to the digits printed."""
    K, steps, dt, every = 3, 4, "0.005", 2
    recv = ("--receiver", "0.5", "0.5", "--receiver", "0.3", "0.71", "0", "--record-every", str(every))
    out = _driver("--ensemble", str(K), "--wave", str(steps), dt, "--direct", *recv)
    lines = re.findall(TRACE_LINE, out, re.M)
    nrec = steps // every + 1
    assert len(lines) == nrec * 2 * K, out
    assert [(int(j), int(q), int(m)) for q, m, j, _, _, _ in lines] == [(j, q, m) for j in range(nrec) for q in range(2) for m in range(K)]
    ens = {(int(q), int(m), int(j)): (t, u, v) for q, m, j, t, u, v in lines}
    assert all(float(ens[(q, m, 0)][1]) == 0.0 and float(ens[(q, m, 0)][2]) == 0.0 for q in range(2) for m in range(K))   # from rest
    assert all(float(ens[(q, m, nrec - 1)][1]) != 0.0 for q in range(2) for m in range(K))
    assert [float(ens[(0, 0, j)][0]) for j in range(nrec)] == [j * every * float(dt) for j in range(nrec)]
    for m in range(K):
        one = re.findall(TRACE_LINE, _driver("--member", str(m), "--wave", str(steps), dt, "--direct", *recv), re.M)
        assert len(one) == nrec * 2
        for q, mm, j, t, u, v in one:
            assert int(mm) == m and ens[(int(q), m, int(j))] == (t, u, v), (m, q, j, ens[(int(q), m, int(j))], (t, u, v))
    assert len({ens[(0, m, nrec - 1)] for m in range(K)}) == K            # the members differ
    # no receiver, no line; the other lines of the run are those of a run without the flags
    plain = _driver("--member", "1", "--wave", str(steps), dt, "--direct")
    with_r = _driver("--member", "1", "--wave", str(steps), dt, "--direct", *recv)
    assert not re.findall(TRACE_LINE, plain, re.M)
    strip = lambda text: [l for l in text.splitlines() if " receiver " not in l and "time" not in l]
    assert strip(plain) == strip(with_r)
