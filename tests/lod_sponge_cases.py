"""Helpers of the tests of the sponge layer, a third damping matrix D in the wave steppers and the frequency response
(slod_lod_newmark_*_damped, slod_lod_factor_create_zldl3, slod_lod_irk_wave_steps_damped_direct,
slod_lod_harmonic_response_damped); a plain module like lod_irk_cases.py, whose cases, dampings, complex yardstick factor,
qualification rule and growth cap it shares.

The model is  M u'' + (dm M + ds A + D) u' + A u = b(t).  The yardsticks, all dense numpy, none calls the library:
  the sponge rule        sigma = sigma_max max(0, 1 - d / width)^2 per cell, d the distance of the cell's centre from the rim
                         of the unit square, width 0.25, sigma_max = 4 sqrt(lam_1) of the case's pencil
  newmark                the damped Newmark loop in acceleration form, numpy.linalg.solve per step
  wave_stage             the damped undiagonalised 4n x 4n stage system (LAPACK's LU), wave_one_solve the one-solve form
  system3                S = alpha A + beta M + gamma D as the scatter kernel rounds it; zldl_reference(system3) is the
                         yardstick factor, qualified as lod_harmonic_cases.qualify qualifies (move up by 1 + 1/64, at most 8
                         times, until no bad pivot and growth <= GROWTH_CAP; none: AssertionError)
  quantities             (u^H M u, u^H A u, u^H D u, Re u^H b, Im u^H b) in np.longdouble
test_lod_sponge_reference.py checks them against each other on the CPU, on the Q1 surrogate of lod_ldl_cases.q1_pencil.
"""
import numpy as np

from lod_harmonic_cases import (FORWARD, GROWTH_CAP, MOVE, MOVES, U, ZBOUND, bound, dampings, rule_frequencies,   # noqa: F401
                                zeta, zldl_reference)
from lod_harmonic_cases import coefficients as harmonic_coefficients
from lod_irk_cases import BUTCHER, GAUSS, LAMBDA, RADAU, SCHEMES, _load, _lu, transform, wave_dts   # noqa: F401
from lod_irk_cases import coefficients as irk_coefficients
from lod_ldl_cases import CASES, q1_pencil   # noqa: F401

WIDTH = 0.25


def sigma_max(lam):
    return 4.0 * float(np.sqrt(lam[0]))


def sponge_sigma(ne, width, smax):
    """[ne][ne] (ey, ex): sigma per cell of an ne x ne grid on the unit square."""
    x = (np.arange(ne) + 0.5) / ne
    d1 = np.minimum(x, 1.0 - x)
    d = np.minimum(d1[:, None], d1[None, :])
    return smax * np.maximum(0.0, 1.0 - d / width) ** 2


def q1_weighted_mass(inner, sigma):
    """The Q1 mass matrix with the weight sigma[ey, ex] per cell on the interior nodes of q1_pencil(inner)."""
    nodes = inner + 2
    ne, h = nodes - 1, 1.0 / (nodes - 1)
    me = np.array([[4, 2, 1, 2], [2, 4, 2, 1], [1, 2, 4, 2], [2, 1, 2, 4]]) * (h * h / 36.0)
    D = np.zeros((nodes * nodes, nodes * nodes))
    for ey in range(ne):
        for ex in range(ne):
            v = [ey * nodes + ex, ey * nodes + ex + 1, (ey + 1) * nodes + ex + 1, (ey + 1) * nodes + ex]
            D[np.ix_(v, v)] += sigma[ey, ex] * me
    keep = np.array([y * nodes + x for y in range(1, nodes - 1) for x in range(1, nodes - 1)])
    return D[np.ix_(keep, keep)]


_q1 = {}


def q1_sponge_case(inner):
    """(A, M, D, lam) of the surrogate with the sponge of the rule; built once."""
    import scipy.linalg as sl
    if inner not in _q1:
        A, M = q1_pencil(inner)
        lam = sl.eigh(A, M, eigvals_only=True)
        D = q1_weighted_mass(inner, sponge_sigma(inner + 1, WIDTH, sigma_max(lam)))
        _q1[inner] = (A, M, D, lam)
    return _q1[inner]


def sponge_dampings(lam):
    """[(label, dm, ds)]: the sponge alone, and the sponge with the Rayleigh pair `both`."""
    both = [d for d in dampings(lam) if d[0] == "both"][0]
    return [("sponge", 0.0, 0.0), ("sponge+both", both[1], both[2])]


# ---- Newmark

def newmark_accel(A, M, D, u, v, b0, dm, ds):
    return np.linalg.solve(M, b0 - A @ (u + ds * v) - dm * (M @ v) - D @ v)


def newmark(A, M, D, dt, beta, gamma, n_steps, u, v, a, loads, dm, ds):
    """(us, vs, as), each [n_steps + 1, ...]; loads(k): the load of level k."""
    Cd = dm * M + ds * A + D
    S = M + gamma * dt * Cd + beta * dt * dt * A
    us, vs, acs = [u], [v], [a]
    for k in range(n_steps):
        ut = u + dt * v + dt * dt * (0.5 - beta) * a
        vt = v + dt * (1.0 - gamma) * a
        a = np.linalg.solve(S, loads(k + 1) - A @ ut - Cd @ vt)
        u, v = ut + beta * dt * dt * a, vt + gamma * dt * a
        us.append(u), vs.append(v), acs.append(a)
    return np.array(us), np.array(vs), np.array(acs)


def energies(A, M, us, vs):
    """(kinetic, potential), [levels][columns]"""
    return 0.5 * np.einsum("kic,ij,kjc->kc", vs, M, vs), 0.5 * np.einsum("kic,ij,kjc->kc", us, A, us)


# ---- IRK

def wave_stage(A, M, D, scheme, dt, n_steps, u0, v0, dm=0.0, ds=0.0, loads=None):
    """lod_irk_cases.wave_stage with C = dm M + ds A + D."""
    Ark, b, _ = BUTCHER[scheme]
    n = A.shape[0]
    Cd = dm * M + ds * A + D
    I2, In = np.eye(2), np.eye(n)
    lu = _lu(np.block([[np.kron(I2, In), -dt * np.kron(Ark, In)],
                       [dt * np.kron(Ark, A), np.kron(I2, M) + dt * np.kron(Ark, Cd)]]))
    u, v = np.array(u0, dtype=np.float64), np.array(v0, dtype=np.float64)
    us, vs = [u], [v]
    for k in range(n_steps):
        f = Cd @ v + A @ u
        rhs = np.concatenate([v, v, _load(loads, k, 0, u.shape) - f, _load(loads, k, 1, u.shape) - f])
        K = lu(rhs)
        u = u + dt * (b[0] * K[:n] + b[1] * K[n:2 * n])
        v = v + dt * (b[0] * K[2 * n:3 * n] + b[1] * K[3 * n:])
        us.append(u), vs.append(v)
    return np.array(us), np.array(vs)


def wave_one_solve(A, M, D, scheme, dt, n_steps, u0, v0, dm=0.0, ds=0.0, loads=None):
    """The one-solve form: S = (1 + z dm) M + (z ds + z^2) A + z D,
    r = tau_1 b_1 + tau_2 b_2 - sigma [A (u + (z + ds) v) + dm M v + D v]."""
    lam, tau, sigma, mu = transform(scheme)
    z = dt * lam
    S = (1.0 + z * dm) * M + (z * ds + z * z) * A + z * D
    u, v = np.array(u0, dtype=np.float64), np.array(v0, dtype=np.float64)
    us, vs = [u], [v]
    for k in range(n_steps):
        r = tau[0] * _load(loads, k, 0, u.shape) + tau[1] * _load(loads, k, 1, u.shape) \
            - sigma * (A @ (u + (z + ds) * v) + dm * (M @ v) + D @ v)
        wv = np.linalg.solve(S, r)
        wu = sigma * v + z * wv
        u, v = u + 2.0 * dt * (mu * wu).real, v + 2.0 * dt * (mu * wv).real
        us.append(u), vs.append(v)
    return np.array(us), np.array(vs)


# ---- the three-term system and its yardstick

def system3(A, M, D, alpha, beta, gamma):
    """alpha A + beta M + gamma D as the scatter kernel rounds it: re = ((a_r A) + (b_r M)) + (g_r D), im alike."""
    alpha, beta, gamma = complex(alpha), complex(beta), complex(gamma)
    return ((alpha.real * A + beta.real * M) + gamma.real * D) + 1j * ((alpha.imag * A + beta.imag * M) + gamma.imag * D)


def harmonic_system(A, M, D, omega, dm, ds):
    alpha, beta = harmonic_coefficients(omega, dm, ds)
    return system3(A, M, D, alpha, beta, 1j * omega)


def irk_system(A, M, D, scheme, dt, dm, ds):
    alpha, beta = irk_coefficients(scheme, 2, dt, dm, ds)
    return system3(A, M, D, alpha, beta, dt * LAMBDA[scheme])


def growth_of(S, perm=None):
    """(growth, yardstick) of the unpivoted complex LDL^T of S in factor order."""
    if perm is not None:
        S = S[np.ix_(perm, perm)]
    ref = zldl_reference(S)
    return (ref.G / ref.norm if ref.bad < 0 else float("inf")), ref


def qualify(A, M, D, omega, dm, ds, perm=None):
    """lod_harmonic_cases.qualify on the three-term system: (omega, yardstick, moves), or AssertionError."""
    seen = []
    for move in range(MOVES + 1):
        g, ref = growth_of(harmonic_system(A, M, D, omega, dm, ds), perm)
        seen.append((omega, ref.bad, g))
        if ref.bad < 0 and g <= GROWTH_CAP:
            return omega, ref, move
        omega *= MOVE
    raise AssertionError("no frequency qualifies: %r" % seen)


def sweep(lam, A, M, D, perm=None):
    """{label: (dm, ds, [(omega, yardstick, moves)])} at the eight rule frequencies and the two sponge dampings."""
    return {label: (dm, ds, [qualify(A, M, D, x, dm, ds, perm) for x in rule_frequencies(lam)])
            for label, dm, ds in sponge_dampings(lam)}


def quantities(A, M, D, u, b):
    """[columns][5] = (u^H M u, u^H A u, u^H D u, Re u^H b, Im u^H b) in np.longdouble, and per column the sum of the moduli
    of the terms of each of the five sums (the scale of their rounding)."""
    ul, bl = u.astype(np.clongdouble), b.astype(np.clongdouble)
    out, mag = [], []
    for X in (M, A, D):
        Xl = X.astype(np.longdouble)
        out.append(np.einsum("ic,ic->c", ul.conj(), Xl @ ul).real)
        mag.append(np.einsum("ic,ic->c", np.abs(ul), np.abs(Xl) @ np.abs(ul)))
    ub = np.einsum("ic,ic->c", ul.conj(), bl)
    m = np.einsum("ic,ic->c", np.abs(ul), np.abs(bl))
    return (np.array(out + [ub.real, ub.imag], dtype=np.longdouble).T, np.array(mag + [m, m], dtype=np.longdouble).T)


# ---- the four GPU cases with their sponge (needs a GPU)

_cases = {}


def sponge_case(so, name):
    """lod_harmonic_cases.harmonic_case(name) with .sigma (host, [NE * NE]), .dvalues (device block rows of D = C^T M_sigma C
    by slod_lod_mass_matrix), .D (dense), .zero_rows (the rows of D that are zero) and .sponge_sweep (the qualified sweep at
    the two sponge dampings); built once.  The conditions on D
    are asserted here: bit-symmetric, smallest eigenvalue >= -1e-12 of the largest."""
    from lod_cases import _mass, _rows_to_dense, _torch
    from lod_harmonic_cases import harmonic_case
    if name not in _cases:
        torch, dev = _torch()
        c = harmonic_case(so, name)
        NE = c.g.NE
        c.sigma = np.ascontiguousarray(sponge_sigma(NE, WIDTH, sigma_max(c.lam_h)).reshape(-1))
        c.sigma_t = torch.from_numpy(c.sigma).to(dev)
        c.dvalues, _ = _mass(c, c.sigma_t)
        c.D = _rows_to_dense(c.g, c.dvalues.cpu().numpy(), c.cols.cpu().numpy().view(np.uint32), c.s)
        assert np.array_equal(c.D, c.D.T), name
        ev = np.linalg.eigvalsh(c.D)
        assert ev[0] >= -1e-12 * ev[-1] and ev[-1] > 0.0, (name, ev[0], ev[-1])
        c.zero_rows = np.nonzero(~c.D.any(axis=1))[0]
        c.sponge_sweep = sweep(c.lam_h, c.A, c.M, c.D, c.perm)       # raises if a frequency does not qualify
        _cases[name] = c
    return _cases[name]
