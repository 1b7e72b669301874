"""The numpy yardstick of the sources on the LOD space (slod_lod_sources_create, slod_lod_inject_*, slod_lod_time_source_arm)
and what the GPU tests of the sources share.  The yardstick works on the CSR rows of a receivers object (row_begin, cols,
values: lod_receiver_cases.receiver_rows, or Receivers.rows() of a handle): the transposed index, b = base + O^T g in
np.longdouble with its S_abs and term count for lod_cases._slab_bar, the densified rows.  Nothing of it calls the library.
Then the six sources of every test, and the ten steppers on fixed matrices and factors with a load argument."""
import numpy as np

import lod_receiver_cases as rc

N_STEPS = 7
SINGLE = ("theta_cg", "theta_direct", "nm_cg", "nm_direct", "irk_heat", "irk_wave")
ENSEMBLE = ("theta_ens", "nm_ens", "irk_heat_ens", "irk_wave_ens")


def six(n, N, s):
    """The six receivers of test_gpu_lod_receivers_time.py as sources: a coarse-cell corner, a cell-interior node, a node
    next to the boundary, a boundary node, a 4-term point (it repeats coarse columns inside a source) and a 2-term
    difference (a negative weight; it shares coarse rows with the first two)."""
    NE = N * n
    NEp = NE + 1
    corner = n * (N // 2) + n * (N // 2) * NEp
    interior = (n + 1) + (2 * n + 1) * NEp
    near = 1 + (NE // 2) * NEp
    boundary = 0 + (NE // 2) * NEp
    return [[(corner, 0, 1.0)], [(interior, s - 1, 1.0)], [(near, 0, 1.0)], [(boundary, s - 1, 1.0)],
            rc.point_terms(NE, 0.43, 0.58, s - 1), [(corner, 0, 1.0), (interior, s - 1, -1.0)]]


def transposed_index(rb, cols, nrow):
    """(rows, begin, perm, q, slot) of the CSR (rb, cols) regrouped by column: the touched coarse rows ascending; slot t owns
    the entries begin[t] .. begin[t+1]-1 of perm, the receivers' entries e with cols[e] = rows[t] in ascending e; q[i] the
    source of entry perm[i]; slot[r] = t or -1."""
    cols = np.asarray(cols, dtype=np.int64)
    src = np.repeat(np.arange(len(rb) - 1), np.diff(np.asarray(rb, dtype=np.int64)))
    rows = np.unique(cols)
    perm = np.argsort(cols, kind="stable")
    begin = np.concatenate([[0], np.cumsum([(cols == r).sum() for r in rows])])
    slot = np.full(nrow, -1, dtype=np.int64)
    slot[rows] = np.arange(len(rows))
    return rows, begin, perm, src[perm], slot


def inject_value(rb, cols, vals, g, nrow, base=None):
    """(b, S_abs, m), each [nrow][columns], of b = base + O^T g in np.longdouble: g [n_src][columns], base [nrow][columns] or
    None; S_abs the same over absolute values, m the entries of the row plus one for the base."""
    g = np.asarray(g).astype(np.longdouble)
    ncol = g.shape[1]
    b = np.zeros((nrow, ncol), dtype=np.longdouble) if base is None else np.asarray(base).astype(np.longdouble).copy()
    sabs = np.abs(b)
    m = np.ones((nrow, ncol), dtype=np.int64)
    for q in range(len(rb) - 1):
        for e in range(int(rb[q]), int(rb[q + 1])):
            r, v = int(cols[e]), np.longdouble(vals[e])
            b[r] += v * g[q]
            sabs[r] += np.abs(v) * np.abs(g[q])
            m[r] += 1
    return b, sabs, m


def dense_rows(rb, cols, vals, nrow):
    """O [n_src][nrow] in float64, equal columns of a row summed."""
    O = np.zeros((len(rb) - 1, nrow))
    for q in range(len(rb) - 1):
        np.add.at(O[q], np.asarray(cols[rb[q]:rb[q + 1]], dtype=np.int64), vals[rb[q]:rb[q + 1]])
    return O


def ricker_closed(t, f0, t0, amp=1.0):
    """The Ricker wavelet written apart from slod_amd.ricker, one time at a time."""
    import math
    a = (math.pi * f0 * (t - t0)) ** 2
    return amp * (1.0 - 2.0 * a) * math.exp(-a)


# ---- the ten steppers (GPU) ----
class Stepper:
    """One of the ten steppers on fixed matrices and a fixed factor: run(state, n_steps, load) advances state (a dict of
    device tensors u, v, a with padded leading dimensions) in place and returns the host outputs of the call; load is None
    or (pointer, ld_load, stride between samples)."""


_steppers = {}


def _state(nrow, ncol, seed, scale_v):
    import lod_irk_ensemble_cases as ec
    rng = np.random.default_rng(seed)
    return {"u": ec.padded(rng.uniform(-1.0, 1.0, (nrow, ncol)), 1), "v": ec.padded(rng.uniform(-1.0, 1.0, (nrow, ncol)) * scale_v, 2),
            "a": ec.nan(nrow, ncol + 1)}


def _ld(load, stage=False):
    if load is None:
        return {}
    return {"d_load": load[0], "ld_load": load[1], "load_stage_stride" if stage else "load_step_stride": load[2]}


def single(so, kind, name="step64", ncol=2):
    import lod_irk_ensemble_cases as ec
    from lod_cases import _pencil
    key = (kind, name, ncol)
    if key in _steppers:
        return _steppers[key]
    c = _pencil(so, name)
    g, cols, A, M = c.g, c.cols.data_ptr(), c.sym.data_ptr(), c.mvalues.data_ptr()
    lam = c.lam
    st = Stepper()
    st.recv = g.lod_receivers(six(g.cfg.n_subdivisions, g.N, c.s), c.b.data_ptr(), c.stride)
    st.src = g.lod_sources(st.recv)
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
        run = lambda s, k, load=None: g.lod_theta_steps(A, M, cols, dt, 0.5, k, s["u"].data_ptr(), n_rhs=ncol, ld_u=s["u"].shape[1], **_ld(load))
    elif kind == "theta_direct":
        dt = 0.1 / lam[0]
        f = comb(1.0, 0.5 * dt)
        run = lambda s, k, load=None: g.lod_theta_steps_direct(f, A, cols, dt, 0.5, k, s["u"].data_ptr(), n_rhs=ncol, ld_u=s["u"].shape[1],
                                                               **_ld(load))
    elif kind == "nm_cg":
        dt = 0.5 / w1
        run = lambda s, k, load=None: g.lod_newmark_steps(A, M, cols, dt, k, s["u"].data_ptr(), s["v"].data_ptr(), s["a"].data_ptr(),
                                                          n_rhs=ncol, **lds(s), **_ld(load))
    elif kind == "nm_direct":
        dt = 0.5 / w1
        f = comb(1.0, 0.25 * dt * dt)
        run = lambda s, k, load=None: g.lod_newmark_steps_direct(f, A, M, cols, dt, k, s["u"].data_ptr(), s["v"].data_ptr(),
                                                                 s["a"].data_ptr(), n_rhs=ncol, **lds(s), **_ld(load))
    elif kind == "irk_heat":
        dt = 0.1 / lam[0]
        f = g.lod_factor_zldl(A, M, cols, *[[x] for x in g.lod_irk_coefficients("radau", 1, dt)])
        run = lambda s, k, load=None: g.lod_irk_heat_steps(f, "radau", A, cols, dt, k, s["u"].data_ptr(), n_rhs=ncol, ld_u=s["u"].shape[1],
                                                           **_ld(load, True))
    else:
        dt = 0.5 / w1
        f = g.lod_factor_zldl(A, M, cols, *[[x] for x in g.lod_irk_coefficients("gauss", 2, dt)])
        run = lambda s, k, load=None: g.lod_irk_wave_steps(f, "gauss", A, M, cols, dt, k, s["u"].data_ptr(), s["v"].data_ptr(), n_rhs=ncol,
                                                           ld_u=s["u"].shape[1], ld_v=s["v"].shape[1], **_ld(load, True))
    st.name, st.g, st.ncol, st.ens, st.run, st.keep = kind, g, ncol, False, run, keep
    st.has_v, st.irk = kind in ("nm_cg", "nm_direct", "irk_wave"), kind.startswith("irk")
    st.state0, st.dt, st.c, st.nrow = st0, dt, c, c.nrow
    _steppers[key] = st
    return st


def ens_slab(c, K):
    """The basis slabs of the K members of lod_irk_ensemble_cases.stack: the three members, then copies."""
    from lod_cases import _torch
    torch, dev = _torch()
    return c.b if K == c.K else torch.cat([c.slab[k % c.K][0] for k in range(K)])


def ensemble(so, kind, name="base", K=3):
    import lod_irk_ensemble_cases as ec
    key = (kind, name, K)
    if key in _steppers:
        return _steppers[key]
    c = ec.ens_case(so, name)
    g, cols = c.g, c.cols.data_ptr()
    At, Mt = ec.stack(c, c.sym, K, 1), ec.stack(c, c.mass, K, 2)
    A, M, lda, ldm = At.data_ptr(), Mt.data_ptr(), K + 1, K + 2
    lam1, lamn = ec.joint_spectrum(c.lam)
    slab = ens_slab(c, K)
    st = Stepper()
    st.recv = g.lod_receivers(six(g.cfg.n_subdivisions, g.N, c.s), slab.data_ptr(), c.stride, n_members=K, member_stride=c.mstride)
    st.src = g.lod_sources(st.recv)
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
        run = lambda s, k, load=None: g.lod_theta_steps_ensemble_direct(f, A, cols, dt, 0.5, k, K, s["u"].data_ptr(), ld_m=lda,
                                                                        ld_u=s["u"].shape[1], **_ld(load))
    elif kind == "nm_ens":
        dt = 0.5 / w1
        fM = comb(1.0, 0.0)
        g.lod_newmark_accel_ensemble_direct(fM, A, M, cols, K, st0["u"].data_ptr(), st0["v"].data_ptr(), st0["a"].data_ptr(), ld_a_m=lda,
                                            ld_m_m=ldm, **lds(st0))
        f = comb(1.0, 0.25 * dt * dt)
        run = lambda s, k, load=None: g.lod_newmark_steps_ensemble_direct(f, A, M, cols, dt, k, K, s["u"].data_ptr(), s["v"].data_ptr(),
                                                                          s["a"].data_ptr(), ld_a_m=lda, ld_m_m=ldm, **lds(s), **_ld(load))
    elif kind == "irk_heat_ens":
        dt = 0.1 / lam1
        a, b = g.lod_irk_coefficients("radau", 1, dt)
        f = g.lod_factor_zldl_ensemble(A, M, cols, K, [a], [b], ld_a_m=lda, ld_b_m=ldm)
        run = lambda s, k, load=None: g.lod_irk_heat_steps_ensemble(f, "radau", A, cols, dt, k, K, s["u"].data_ptr(), ld_a_m=lda,
                                                                    ld_u=s["u"].shape[1], **_ld(load, True))
    else:
        dt = 0.5 / w1
        a, b = g.lod_irk_coefficients("gauss", 2, dt)
        f = g.lod_factor_zldl_ensemble(A, M, cols, K, [a], [b], ld_a_m=lda, ld_b_m=ldm)
        run = lambda s, k, load=None: g.lod_irk_wave_steps_ensemble(f, "gauss", A, M, cols, dt, k, K, s["u"].data_ptr(), s["v"].data_ptr(),
                                                                    ld_a_m=lda, ld_m_m=ldm, ld_u=s["u"].shape[1], ld_v=s["v"].shape[1],
                                                                    **_ld(load, True))
    st.name, st.g, st.ncol, st.ens, st.run, st.keep = kind, g, K, True, run, keep
    st.has_v, st.irk = kind in ("nm_ens", "irk_wave_ens"), kind.startswith("irk")
    st.state0, st.dt, st.c, st.nrow = st0, dt, c, c.nrow
    _steppers[key] = st
    return st


def get(so, kind, **kw):
    return single(so, kind, **kw) if kind in SINGLE else ensemble(so, kind, **kw)
