"""GPU tests of the source of the time loops on the LOD space (slod_lod_time_source_arm) on real pencils (lod_cases._pencil:
step64, s2, rowmajor) and on the ensemble configurations of lod_irk_ensemble_cases, with the six sources of
lod_source_cases.six, n_steps = 7 and signals random in [-1, 1] per (sample, source, column).

For each of the ten steppers, without a base load, with a constant one and with one per step: the armed call leaves in
every output the words of an un-armed call whose d_load holds the loads materialised by slod_lod_inject_*, sample by
sample, and two armed steps are twice one armed step with the signal advanced.  Then source and record armed together, the
one-shot rule, every source refusal by message and order, the ensemble against the single stepper per member (K = 3 and
K = 65), the states against dense numpy recursions with the loads O_dense^T g within lod_irk_cases.FORWARD = 1e-8 of
max |reference|, and reciprocity of a Ricker source between two points.

Measured on an MI355X (printed by the tests; DESIGN section 6, "Sources"): worst |state - dense recursion| / max |reference|
of test_against_the_dense_recursion 1.2e-14 (theta CG 6.6e-15, theta factor 6.1e-16, Newmark CG 4.8e-15, Newmark factor
3.7e-15, Radau heat 3.3e-16, Gauss wave 1.2e-14) against the bar 1e-8.  Reciprocity: max |trace_B(A) - trace_A(B)| /
max |trace| 1.1e-14 on the trapezoidal factor stepper and 1.6e-15 on Gauss IRK, against the tolerance 2e-8."""
import os
import re
import subprocess

import numpy as np
import pytest

import lod_irk_cases as ic
import lod_irk_ensemble_cases as ec
import lod_source_cases as sc
from lod_cases import _bits, _torch
from lod_source_cases import ENSEMBLE, N_STEPS, SINGLE

pytestmark = pytest.mark.gpu

SENT_BITS = 0x5a5a5a5a5a5a5a5a
SENT = np.array([SENT_BITS], dtype=np.uint64).view(np.float64)[0]
U, V = 1, 2
NSRC = 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")


def _sync():
    _torch()[0].cuda.synchronize()


def _sent(*shape):
    torch, dev = _torch()
    return torch.full(shape, float(SENT), dtype=torch.float64, device=dev)


def _clone(state):
    return {k: t.clone() for k, t in state.items()}


def _host(extra):
    if extra is None:
        return ()
    out = []
    for a in (extra if isinstance(extra, tuple) else (extra,)):
        if a is not None:
            a = np.ascontiguousarray(a)
            out.append(a.view(np.uint64) if a.dtype == np.float64 else a.copy())
    return tuple(out)


def _run(st, n_steps, arm=None, load=None, state=None):
    """A call from the entry state (or `state`, advanced in place); arm() is called right before it.  Returns (state words,
    host outputs, state)."""
    s = _clone(st.state0) if state is None else state
    if arm is not None:
        arm()
    extra = st.run(s, n_steps, load)
    _sync()
    return {k: _bits(t) for k, t in s.items()}, _host(extra), s


def _same(a, b):
    return all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def _need(st, n_steps=N_STEPS):
    return 2 * n_steps if st.irk else n_steps + 1


def _per_step(st):
    return 2 if st.irk else 1


class _Signal:
    """[samples][sources][columns] on the device with sentinel padding in ld_signal and between samples, and a spare sample."""

    def __init__(self, st, values=None, seed=71, src=None, nsrc=NSRC):
        self.st, self.src = st, st.src if src is None else src
        self.ns = _need(st)
        self.h = np.random.default_rng(seed).uniform(-1.0, 1.0, (self.ns, nsrc, st.ncol)) if values is None else values
        self.ld = st.ncol + 1
        self.stride = nsrc * self.ld + 3
        self.t = _sent((self.ns + 1) * self.stride)
        for j in range(self.ns):
            self.t[j * self.stride:j * self.stride + nsrc * self.ld].view(nsrc, self.ld)[:, :st.ncol] = ec.dev(self.h[j])

    def ptr(self, sample=0):
        return self.t.data_ptr() + 8 * sample * self.stride

    def arm(self, first=0, **kw):
        a = dict(n_samples=self.ns - first, ld_signal=self.ld, sample_stride=self.stride)
        a.update(kw)
        return self.st.g.lod_time_source(self.src, self.ptr(first), **a)


class _Base:
    """The caller's own load of a stepper call: none, constant (stride 0) or one per sample, NaN in the padding."""

    def __init__(self, st, kind, seed=72):
        self.kind, ns = kind, _need(st)
        self.ld = st.ncol + 2
        rng = np.random.default_rng(seed)
        if kind == "none":
            self.t, self.stride = None, 0
        elif kind == "const":
            self.t, self.stride = ec.padded(rng.uniform(-1.0, 1.0, (st.nrow, st.ncol)), 2), 0
        else:
            self.stride = st.nrow * self.ld + 5
            self.t = ec.nan(ns * self.stride)
            for j in range(ns):
                self.t[j * self.stride:j * self.stride + st.nrow * self.ld].view(st.nrow, self.ld)[:, :st.ncol] = \
                    ec.dev(rng.uniform(-1.0, 1.0, (st.nrow, st.ncol)))

    def ptr(self, sample=0):
        return None if self.t is None else self.t.data_ptr() + 8 * sample * self.stride

    def load(self, first=0):
        return None if self.t is None else (self.ptr(first), self.ld, self.stride)

    def host(self, st, sample):
        if self.t is None:
            return np.zeros((st.nrow, st.ncol))
        off = sample * self.stride
        return self.t[off:off + st.nrow * self.ld].view(st.nrow, self.ld)[:, :st.ncol].cpu().numpy()


def _materialise(st, sig, base):
    """The loads base + O^T g of every sample by slod_lod_inject_*, as a d_load of the un-armed call."""
    ld = st.ncol + 3
    stride = st.nrow * ld + 1
    L = ec.nan(sig.ns * stride)
    for j in range(sig.ns):
        kw = dict(d_base=base.ptr(j), ld_g=sig.ld, ld_base=base.ld, ld_b=ld)
        if st.ens:
            sig.src.inject_ensemble(sig.ptr(j), L.data_ptr() + 8 * j * stride, n_members=st.ncol, **kw)
        else:
            sig.src.inject(sig.ptr(j), L.data_ptr() + 8 * j * stride, n_rhs=st.ncol, **kw)
    _sync()
    return L, (L.data_ptr(), ld, stride)


CASES = [(kind, name) for kind in SINGLE for name in ("step64", "s2", "rowmajor")] + [(kind, name) for kind in ENSEMBLE for name in ec.NAMES]


@pytest.mark.parametrize("kind,name", CASES)
def test_armed_call_equals_the_call_on_materialised_loads(so, kind, name):
    st = sc.get(so, kind, name=name)
    sig = _Signal(st)
    plain = _run(st, N_STEPS)
    for bkind in ("none", "const", "steps"):
        base = _Base(st, bkind)
        L, load = _materialise(st, sig, base)
        want = _run(st, N_STEPS, load=load)
        armed = _run(st, N_STEPS, sig.arm, base.load())
        assert _same(want, armed), (kind, name, bkind)
        assert not _same(plain, armed) and np.isfinite(armed[2]["u"][:, :st.ncol].cpu().numpy()).all()
        # two armed steps are twice one armed step with the signal (and the caller's loads) advanced
        two = _run(st, 2, sig.arm, base.load())
        s = _clone(st.state0)
        for k in range(2):
            first = k * _per_step(st)
            one = _run(st, 1, lambda: sig.arm(first=first), base.load(first if bkind == "steps" else 0), state=s)
        assert all(np.array_equal(two[0][q], one[0][q]) for q in two[0]), (kind, name, bkind)
    assert (_bits(sig.t[sig.ns * sig.stride:]) == SENT_BITS).all()


@pytest.mark.parametrize("kind", SINGLE + ENSEMBLE)
def test_source_and_record_together(so, kind):
    """The trace of a driven loop has the words of slod_lod_observe_* on the states that separate driven calls of
    0 .. n_steps steps leave; every other word of d_trace keeps its sentinel."""
    st = sc.get(so, kind)
    sig = _Signal(st)
    nq, nr, nc = (2 if st.has_v else 1), st.recv.n_recv, st.ncol
    trace = _sent(N_STEPS + 2, nq, nr, nc + 1)
    st.g.lod_time_record(st.recv, trace.data_ptr(), capacity=N_STEPS + 1, what=U | V if st.has_v else U, ld_trace=nc + 1)
    driven = _run(st, N_STEPS, sig.arm)
    want = np.full(trace.shape, SENT_BITS, dtype=np.uint64)

    def observe(x):
        y = _sent(nr, nc)
        if st.ens:
            st.recv.observe_ensemble(x.data_ptr(), y.data_ptr(), n_members=nc, ld_u=x.shape[1])
        else:
            st.recv.observe(x.data_ptr(), y.data_ptr(), n_rhs=nc, ld_u=x.shape[1])
        _sync()
        return _bits(y)

    for j in range(N_STEPS + 1):
        s = _clone(st.state0) if j == 0 else _run(st, j, sig.arm)[2]
        want[j, 0, :, :nc] = observe(s["u"])
        if st.has_v:
            want[j, 1, :, :nc] = observe(s["v"])
    assert np.array_equal(_bits(trace), want), kind
    # and the record does not perturb the driven call
    assert _same(driven, _run(st, N_STEPS, sig.arm))


@pytest.mark.parametrize("kind", SINGLE + ENSEMBLE)
def test_one_shot(so, kind):
    import slod_amd
    st = sc.get(so, kind)
    sig = _Signal(st)
    plain = _run(st, N_STEPS)
    driven = _run(st, N_STEPS, sig.arm)
    assert not _same(plain, driven)
    assert _same(plain, _run(st, N_STEPS))                                # the next call runs un-driven
    # a call refused by one of its own checks consumes the arming
    sig.arm()
    with pytest.raises(slod_amd.SlodError) as e:
        st.run(_clone(st.state0), 0)
    assert e.value.code == -1 and "n_steps < 1" in str(e.value)
    assert _same(plain, _run(st, N_STEPS))
    # so does a source refusal
    sig.arm(n_samples=1)
    with pytest.raises(slod_amd.SlodError) as e:
        st.run(_clone(st.state0), N_STEPS)
    assert "source: n_samples below" in str(e.value)
    assert _same(plain, _run(st, N_STEPS))
    # disarming by hand
    sig.arm()
    st.g.lod_time_source(None, 0)
    assert _same(plain, _run(st, N_STEPS))
    # destroying the sources a source names disarms it
    gone = st.g.lod_sources(st.recv)
    _Signal(st, values=sig.h, src=gone).arm()
    gone.close()
    assert _same(plain, _run(st, N_STEPS))
    # a source and a record are taken together: a record armed alone does not keep a later source from the next call
    trace = _sent(N_STEPS + 1, 2 if st.has_v else 1, st.recv.n_recv, st.ncol)
    st.g.lod_time_record(st.recv, trace.data_ptr(), capacity=N_STEPS + 1, columns=st.ncol)
    assert _same(plain, _run(st, N_STEPS))
    assert _same(driven, _run(st, N_STEPS, sig.arm))


def test_other_calls_do_not_consume_the_arming(so):
    st = sc.single(so, "nm_direct")
    c, g = st.c, st.g
    sig = _Signal(st)
    driven = _run(st, N_STEPS, sig.arm)
    sig.arm()
    fM = g.lod_factor(c.mvalues.data_ptr(), c.cols.data_ptr())
    s = _clone(st.state0)
    acc, y, b = ec.nan(c.nrow, st.ncol + 1), ec.nan(c.nrow, st.ncol), ec.nan(c.nrow, st.ncol)
    g.lod_newmark_accel_direct(fM, c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), s["u"].data_ptr(), s["v"].data_ptr(),
                               acc.data_ptr(), n_rhs=st.ncol, ld_u=s["u"].shape[1], ld_v=s["v"].shape[1], ld_a=acc.shape[1])
    g.lod_newmark_accel(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), s["u"].data_ptr(), s["v"].data_ptr(), acc.data_ptr(),
                        n_rhs=st.ncol, ld_u=s["u"].shape[1], ld_v=s["v"].shape[1], ld_a=acc.shape[1])
    g.lod_apply(c.sym.data_ptr(), c.cols.data_ptr(), s["u"].data_ptr(), y.data_ptr(), n_rhs=st.ncol, ld_x=s["u"].shape[1])
    st.src.inject(sig.ptr(0), b.data_ptr(), n_rhs=st.ncol, ld_g=sig.ld)
    _sync()
    assert _same(driven, _run(st, N_STEPS))                                # still armed
    fM.close()


@pytest.mark.parametrize("kind", SINGLE + ENSEMBLE)
def test_source_refusals(so, kind):
    import slod_amd
    st = sc.get(so, kind)
    sig = _Signal(st)
    nc, c = st.ncol, st.c
    cols_word = "n_members" if st.ens else "n_rhs"
    bound = "2 n_steps" if st.irk else "n_steps + 1"
    other = sc.single(so, "theta_direct", name="rowmajor").src              # a handle of its own
    terms = sc.six(st.g.cfg.n_subdivisions, st.g.N, c.s)
    if st.ens:
        wr = st.g.lod_receivers(terms, c.b.data_ptr(), c.stride)
    else:
        wr = st.g.lod_receivers(terms, c.b.data_ptr(), c.stride, n_members=2, member_stride=0)
    wrong = st.g.lod_sources(wr)
    # the faults in the order of the checks; fault i together with every later one is reported as fault i
    faults = [(dict(ptr=0), "source: NULL d_signal"),
              (dict(ld_signal=nc - 1), "source: ld_signal below " + cols_word),
              (dict(sample_stride=NSRC * sig.ld - 1), "source: sample_stride below n_sources ld_signal"),
              (dict(n_samples=_need(st) - 1), "source: n_samples below " + bound),
              (dict(src=other), "source: sources of another handle"),
              (dict(src=wrong), "source: sources of another member count")]

    def arm(kw):
        a = dict(n_samples=sig.ns, ld_signal=sig.ld, sample_stride=sig.stride)
        a.update({k: v for k, v in kw.items() if k not in ("ptr", "src")})
        st.g.lod_time_source(kw.get("src", st.src), kw.get("ptr", sig.ptr()), **a)

    def refused(kw, word, n_steps=N_STEPS):
        s = _clone(st.state0)
        arm(kw)
        with pytest.raises(slod_amd.SlodError) as e:
            st.run(s, n_steps)
        assert e.value.code == -1 and word in str(e.value) and "slod_lod_" in str(e.value), (kw, str(e.value))
        _sync()
        assert all(np.array_equal(_bits(s[k]), _bits(st.state0[k])) for k in s)      # the state is untouched

    for i, (kw, word) in enumerate(faults):
        refused(kw, word)
        both = dict(kw)
        for later, _ in faults[i + 1:]:
            if not ("src" in both and "src" in later):
                both.update(later)
        refused(both, word)
    refused(dict(sample_stride=0), "source: sample_stride below n_sources ld_signal")
    refused(dict(n_samples=0), "source: n_samples below " + bound)
    # the record's refusals come before the source's, the stepper's own before both
    st.g.lod_time_record(st.recv, 0, capacity=N_STEPS + 1, every=0, columns=nc)
    refused(dict(ptr=0), "record: every < 1")
    arm(dict(ptr=0))
    with pytest.raises(slod_amd.SlodError) as e:
        st.run(_clone(st.state0), -1)
    assert "source" not in str(e.value) and "record" not in str(e.value)
    # exactly enough is taken
    plain = _run(st, N_STEPS)
    driven = _run(st, N_STEPS, lambda: arm(dict(n_samples=_need(st))))
    assert not _same(plain, driven)
    wrong.close(), wr.close()


def _member_single(so, ens, k, sig):
    """The single stepper of member k of an ensemble stepper, driven by column k of the signal: de-interleaved matrices, a
    one-member factor, one-member sources on member k's slab; the state is column k."""
    c, g, K, kind, dt = ens.c, ens.g, ens.ncol, ens.name, ens.dt
    f = ec.scale(K, k, c.K)
    Ak, Mk = (c.sym[k % c.K] * f).contiguous(), (c.mass[k % c.K] * f).contiguous()
    A, M, cols = Ak.data_ptr(), Mk.data_ptr(), c.cols.data_ptr()
    recv = g.lod_receivers(sc.six(g.cfg.n_subdivisions, g.N, c.s), c.slab[k % c.K][0].data_ptr(), c.stride)
    src = g.lod_sources(recv)
    s = {n: t[:, k:k + 1].contiguous() for n, t in ens.state0.items()}
    col = ec.dev(sig.h[:, :, k:k + 1])
    g.lod_time_source(src, col.data_ptr(), n_samples=sig.ns)

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
    fk.close(), recv.close(), src.close()
    return {n: _bits(t)[:, 0] for n, t in s.items()}


@pytest.mark.parametrize("K", (3, 65))
@pytest.mark.parametrize("kind", ENSEMBLE)
def test_ensemble_equals_the_single_stepper_per_member(so, kind, K):
    st = sc.ensemble(so, kind, K=K)
    sig = _Signal(st)
    got = _run(st, N_STEPS, sig.arm)[0]
    used = ("u", "v", "a") if kind == "nm_ens" else ("u", "v") if st.has_v else ("u",)
    for k in range(K):
        one = _member_single(so, st, k, sig)
        for q in used:
            assert np.array_equal(got[q][:, k], one[q]), (kind, K, k, q)


def _dense_states(kind, A, M, dt, u, v, a, b):
    """The state after N_STEPS of the dense recursion of a scheme with the loads b [samples]: theta = 1/2 (b^k), the
    trapezoidal rule in acceleration form (b^(k+1) in step k), or the undiagonalised stage system of lod_irk_cases."""
    if kind.startswith("theta"):
        S = M + 0.5 * dt * A
        for k in range(N_STEPS):
            u = u + np.linalg.solve(S, dt * (0.5 * b[k + 1] + 0.5 * b[k] - A @ u))
        return u, None
    if kind.startswith("nm"):
        S = M + 0.25 * dt * dt * A
        for k in range(N_STEPS):
            ut, vt = u + dt * v + 0.25 * dt * dt * a, v + 0.5 * dt * a
            a = np.linalg.solve(S, b[k + 1] - A @ ut)
            u, v = ut + 0.25 * dt * dt * a, vt + 0.5 * dt * a
        return u, v
    if kind == "irk_heat":
        return ic.heat_stage(A, M, ic.RADAU, dt, N_STEPS, u, loads=b)[-1], None
    us, vs = ic.wave_stage(A, M, ic.GAUSS, dt, N_STEPS, u, v, loads=b)
    return us[-1], vs[-1]


@pytest.mark.parametrize("kind", SINGLE)
def test_against_the_dense_recursion(so, kind):
    """theta on CG and on a factor, Newmark on CG and on a factor, Radau heat and Gauss wave: the state after 7 driven steps
    against the dense recursion with the loads O_dense^T g, within lod_irk_cases.FORWARD = 1e-8 of max |reference|."""
    st = sc.single(so, kind)
    c = st.c
    sig = _Signal(st)
    got = _run(st, N_STEPS, sig.arm)[2]
    O = sc.dense_rows(*st.recv.rows(), c.nrow)
    b = np.einsum("qr,jqc->jrc", O, sig.h)
    h = {k: t[:, :st.ncol].cpu().numpy() for k, t in st.state0.items()}
    u, v = _dense_states(kind, c.A, c.M, st.dt, h["u"], h["v"], h["a"], b)
    plain = _run(st, N_STEPS)[2]
    worst = 0.0
    for name, ref in (("u", u), ("v", v)):
        if ref is None:
            continue
        x = got[name][:, :st.ncol].cpu().numpy()
        worst = max(worst, np.abs(x - ref).max() / np.abs(ref).max())
        # the source matters at this bar: the un-driven state is far from the reference
        assert np.abs(plain[name][:, :st.ncol].cpu().numpy() - ref).max() / np.abs(ref).max() > 1e3 * ic.FORWARD
    print("driven state against the dense recursion, %s: worst |x - ref| / max |reference| = %.3e" % (kind, worst))
    assert worst <= ic.FORWARD, (kind, worst)


@pytest.mark.parametrize("kind", ("nm_direct", "irk_wave"))
def test_reciprocity(so, kind):
    """step64, bit-symmetric sym(A) and M, from rest: the u-trace at B of a Ricker source at A equals the trace at A of the
    same source at B, within 2 FORWARD max |trace| (each side is within FORWARD of the same dense recursion, whose
    propagator is self-adjoint in the pair)."""
    import slod_amd
    torch, dev = _torch()
    st = sc.single(so, kind)
    c, g, nc = st.c, st.g, st.ncol
    terms = sc.six(g.cfg.n_subdivisions, g.N, c.s)
    pair = g.lod_receivers([terms[1], terms[4]], c.b.data_ptr(), c.stride)      # A: an interior node, B: a 4-term point
    src = g.lod_sources(pair)
    ns = _need(st)
    if st.irk:
        cs = ic.BUTCHER[ic.GAUSS][2]
        times = np.array([(k + cs[i]) * st.dt for k in range(N_STEPS) for i in range(2)])
    else:
        times = np.arange(ns) * st.dt
    w = slod_amd.ricker(times, 1.0 / (4.0 * st.dt), 3.0 * st.dt)
    traces = []
    for at in (0, 1):
        h = np.zeros((ns, 2, nc))
        h[:, at, :] = w[:, None]
        sig = _Signal(st, values=h, src=src, nsrc=2)
        s = {k: torch.zeros_like(t) for k, t in st.state0.items()}
        if kind == "nm_direct":                                            # M a^0 = b^0
            b0 = ec.nan(c.nrow, nc)
            src.inject(sig.ptr(0), b0.data_ptr(), n_rhs=nc, ld_g=sig.ld)
            g.lod_newmark_accel(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), s["u"].data_ptr(), s["v"].data_ptr(),
                                s["a"].data_ptr(), n_rhs=nc, ld_u=s["u"].shape[1], ld_v=s["v"].shape[1], ld_a=s["a"].shape[1],
                                d_load=b0.data_ptr(), ld_load=nc)
        trace = _sent(N_STEPS + 1, 2, nc)
        g.lod_time_record(pair, trace.data_ptr(), capacity=N_STEPS + 1, columns=nc)
        _run(st, N_STEPS, sig.arm, state=s)
        traces.append(trace.cpu().numpy()[:, 1 - at, :])
    top = max(np.abs(traces[0]).max(), np.abs(traces[1]).max())
    diff = np.abs(traces[0] - traces[1]).max()
    print("reciprocity, %s: max |trace_B(A) - trace_A(B)| = %.3e, max |trace| = %.3e, ratio %.3e" % (kind, diff, top, diff / top))
    assert top > 0.0 and diff <= 2.0 * ic.FORWARD * top, (kind, diff, top)
    pair.close(), src.close()


TRACE_LINE = r"^wave receiver (\d+) member (\d+) record (\d+): t = (\S+), u = (\S+), v = (\S+)$"


def test_driver_source_lines(so):
    """main_Diffusion 3 2 1 1 --wave 8 DT --direct --source .. --source .. --ricker F0 T0 AMP --quiet-load --receiver ..
    --receiver ..: the receiver lines are those of the Python path (the driver's coefficient Alpha(1, 100, 3), srand(1); from
    rest, M a^0 = O^T g(0), the trapezoidal rule on the factor, one armed call) to the digits printed: within one unit of the
    twelfth decimal of the mantissa, the last one of the driver's %.12e (the two paths round the wavelet on their own)."""
    import slod_amd
    from lod_cases import _build, _mass, _symmetrize
    torch, dev = _torch()
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    steps, dt, f0, t0, amp = 8, 0.005, 40.0, 0.015, 2.5
    spts, rpts = [(0.5, 0.5, 0), (0.3, 0.71, 0)], [(0.25, 0.5, 0), (0.62, 0.4, 0)]
    flags = []
    for x, y, comp in spts:
        flags += ["--source", str(x), str(y), str(comp)]
    for x, y, comp in rpts:
        flags += ["--receiver", str(x), str(y), str(comp)]
    r = subprocess.run([BIN, "3", "2", "1", "1", "--wave", str(steps), str(dt), "--direct", "--ricker", str(f0), str(t0), str(amp),
                        "--quiet-load", *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = re.findall(TRACE_LINE, r.stdout, re.M)
    assert len(lines) == (steps + 1) * len(rpts), r.stdout
    # the Python path
    kw = dict(nref=3, n_sub=2, oversampling=1, spacedim=1)
    cfg = so.make_cfg(stabilize=1, **{k: v for k, v in kw.items() if k != "spacedim"})
    c = _build(so, kw, fields=[so.fill_coefficient_rand(1.0, 100.0, 3, so.n_cells_per_side(cfg) * 2, seed=1)])
    g = c.g
    c.mvalues, _ = _mass(c)
    sym = _symmetrize(c)
    A, M, cols = sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr()
    recv = g.lod_receivers([slod_amd.point_terms(g.NE, 1, *p) for p in rpts], c.b.data_ptr(), c.stride)
    srcr = g.lod_receivers([slod_amd.point_terms(g.NE, 1, *p) for p in spts], c.b.data_ptr(), c.stride)
    src = g.lod_sources(srcr)
    w = slod_amd.ricker(np.arange(steps + 1) * dt, f0, t0, amp)
    sig = ec.dev(np.repeat(w[:, None], len(spts), axis=1).reshape(steps + 1, len(spts), 1))
    u, v, a = (torch.zeros(c.nrow, 1, dtype=torch.float64, device=dev) for _ in range(3))
    b0 = ec.nan(c.nrow, 1)
    src.inject(sig.data_ptr(), b0.data_ptr())
    fM = g.lod_factor(M, cols)
    g.lod_newmark_accel_direct(fM, A, M, cols, u.data_ptr(), v.data_ptr(), a.data_ptr(), d_load=b0.data_ptr(), ld_load=1)
    S = ec.nan(sym.numel())
    g.lod_matrix_combine(1.0, M, 0.25 * dt * dt, A, S.data_ptr())
    _sync()
    f = g.lod_factor(S.data_ptr(), cols)
    trace = _sent(steps + 1, 2, len(rpts))
    g.lod_time_record(recv, trace.data_ptr(), capacity=steps + 1, what=U | V)
    g.lod_time_source(src, sig.data_ptr(), n_samples=steps + 1)
    g.lod_newmark_steps_direct(f, A, M, cols, dt, steps, u.data_ptr(), v.data_ptr(), a.data_ptr(), energies=False)
    _sync()
    t = trace.cpu().numpy()
    assert np.abs(t[-1, 0]).min() > 0.0

    def same_digits(text, value):
        unit = 10.0 ** (np.floor(np.log10(abs(value))) - 12) if value != 0.0 else 0.0
        return abs(float(text) - value) <= unit

    for q, m, j, tt, uu, vv in lines:
        q, j = int(q), int(j)
        assert int(m) == 0 and float(tt) == j * dt
        assert same_digits(uu, t[j, 0, q]) and same_digits(vv, t[j, 1, q]), (q, j, uu, vv, t[j, :, q])
    # the problem's own load is dropped: without the sources nothing moves
    quiet = subprocess.run([BIN, "3", "2", "1", "1", "--wave", "2", str(dt), "--direct", "--quiet-load", *flags[4 * len(spts):]],
                           capture_output=True, text=True, timeout=300)
    assert quiet.returncode == 0, quiet.stderr
    assert all(float(uu) == 0.0 and float(vv) == 0.0 for _, _, _, _, uu, vv in re.findall(TRACE_LINE, quiet.stdout, re.M))
    for o in (fM, f, recv, srcr, src):
        o.close()
    g.close()
