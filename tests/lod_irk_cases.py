"""Helpers of the tests of the two-stage implicit Runge-Kutta steppers on the LOD space (slod_lod_irk_coefficients,
slod_lod_irk_heat_steps_direct, slod_lod_irk_wave_steps_direct); a plain module like lod_harmonic_cases.py, whose cases,
dampings, complex yardstick factor and growth cap it shares.

The yardstick is the undiagonalised stage system in numpy float64: for y' = J y + g(t) the stages K_i solve
  (I - dt A_rk (x) J) K = 1 (x) (J y) + G,   y+ = y + dt sum_i b_i K_i,
written for heat (2n x 2n, multiplied through by M) and wave (4n x 4n in (u, v)) and solved by LAPACK's LU with partial
pivoting (what numpy.linalg.solve runs; factored once per run).  The
one-solve form (one complex system per step, what the library runs) is written here a second time in numpy complex128
from the eigen-decomposition numpy computes of A_rk, so test_lod_irk_reference.py checks the transformation on the CPU.
The Pade stability functions give the third, closed-form reference for single modes.  Nothing here calls the library.

The rule for dt, per case (lam the ascending spectrum of (sym A, M)):
  heat  0.1 / lam_1,  1 / sqrt(lam_1 lam_n),  10 / lam_1
  wave  0.5 / sqrt(lam_1),  0.05 / sqrt(lam_1),  2 / sqrt(lam_n)
Bars: FORWARD = 1e-8 of max |reference| (the project's bar for a solve against a dense reference); the growth of every
step matrix <= GROWTH_CAP = 1e4 as a condition before the library is called.
"""
import numpy as np

from lod_harmonic_cases import FORWARD, GROWTH_CAP, combined, dampings, zldl_reference   # noqa: F401
from lod_ldl_cases import CASES, q1_pencil   # noqa: F401

GAUSS, RADAU = 0, 1
SCHEMES = (("gauss", GAUSS), ("radau", RADAU))
R3, R2 = np.sqrt(3.0), np.sqrt(2.0)
BUTCHER = {
    GAUSS: (np.array([[0.25, 0.25 - R3 / 6.0], [0.25 + R3 / 6.0, 0.25]]), np.array([0.5, 0.5]),
            np.array([0.5 - R3 / 6.0, 0.5 + R3 / 6.0])),
    RADAU: (np.array([[5.0 / 12.0, -1.0 / 12.0], [0.75, 0.25]]), np.array([0.75, 0.25]), np.array([1.0 / 3.0, 1.0])),
}
LAMBDA = {GAUSS: 0.25 + 1j * R3 / 12.0, RADAU: 1.0 / 3.0 + 1j * R2 / 6.0}


def stability(scheme, x):
    """The Pade approximant R(x) of exp(x) that is the scheme's stability function; x scalar, array or square matrix
    (a matrix argument gives the matrix function, the amplification matrix of a linear system)."""
    if np.ndim(x) == 2:
        I = np.eye(x.shape[0])
        if scheme == GAUSS:
            return np.linalg.solve(I - x / 2.0 + x @ x / 12.0, I + x / 2.0 + x @ x / 12.0)
        return np.linalg.solve(I - 2.0 * x / 3.0 + x @ x / 6.0, I + x / 3.0)
    if scheme == GAUSS:
        return (1.0 + x / 2.0 + x * x / 12.0) / (1.0 - x / 2.0 + x * x / 12.0)
    return (1.0 + x / 3.0) / (1.0 - 2.0 * x / 3.0 + x * x / 6.0)


def wave_amplification(scheme, dt, lam, dm, ds):
    """The 2 x 2 matrix that carries the modal (u, v) of eigenvalue lam = omega^2 over one step."""
    return stability(scheme, dt * np.array([[0.0, 1.0], [-lam, -(dm + ds * lam)]]))


def heat_dts(lam):
    return [0.1 / lam[0], 1.0 / np.sqrt(lam[0] * lam[-1]), 10.0 / lam[0]]


def wave_dts(lam):
    return [0.5 / np.sqrt(lam[0]), 0.05 / np.sqrt(lam[0]), 2.0 / np.sqrt(lam[-1])]


def wave_dampings(lam):
    """Undamped, then the three of lod_harmonic_cases.dampings."""
    return [("none", 0.0, 0.0)] + dampings(lam)


def coefficients(scheme, order, dt, dm=0.0, ds=0.0):
    """(alpha, beta) of S = alpha A + beta M from the closed-form lambda, in numpy complex128."""
    z = dt * LAMBDA[scheme]
    return (z, 1.0 + 0.0j) if order == 1 else (z * ds + z * z, 1.0 + z * dm)


def step_matrix(A, M, scheme, order, dt, dm=0.0, ds=0.0):
    """S as the factor's scatter kernel rounds it from the closed-form coefficients."""
    alpha, beta = coefficients(scheme, order, dt, dm, ds)
    return combined(A, M, alpha, beta)


def _load(loads, k, i, shape):
    """loads: None (zero), an array of the state's shape (constant) or [2 n_steps, ...] stage loads."""
    if loads is None:
        return np.zeros(shape)
    return loads if loads.shape == shape else loads[2 * k + i]


def _lu(big):
    """numpy.linalg.solve with the one matrix of a run: LAPACK's getrf once, getrs per step (numpy.linalg.solve is the
    two in one call)."""
    import scipy.linalg as sl
    fac = sl.lu_factor(big)
    return lambda rhs: sl.lu_solve(fac, rhs)


def heat_stage(A, M, scheme, dt, n_steps, u0, loads=None):
    """[n_steps + 1, ...] states of the undiagonalised 2n x 2n stage system  (I (x) M + dt A_rk (x) A) K = G - 1 (x) A u."""
    Ark, b, _ = BUTCHER[scheme]
    n = A.shape[0]
    lu = _lu(np.kron(np.eye(2), M) + dt * np.kron(Ark, A))
    u, out = np.array(u0, dtype=np.float64), [np.array(u0, dtype=np.float64)]
    for k in range(n_steps):
        g = A @ u
        rhs = np.concatenate([_load(loads, k, 0, u.shape) - g, _load(loads, k, 1, u.shape) - g])
        K = lu(rhs)
        u = u + dt * (b[0] * K[:n] + b[1] * K[n:])
        out.append(u)
    return np.array(out)


def wave_stage(A, M, scheme, dt, n_steps, u0, v0, dm=0.0, ds=0.0, loads=None):
    """([n_steps + 1, ...] u, the same of v) of the undiagonalised 4n x 4n stage system in (u, v): stage derivatives
    (Ku_i, Kv_i) with  Ku_i = v + dt sum a_ij Kv_j,  M Kv_i = b_i - C (v + dt sum a_ij Kv_j) - A (u + dt sum a_ij Ku_j)."""
    Ark, b, _ = BUTCHER[scheme]
    n = A.shape[0]
    Cd = dm * M + ds * A
    I2, In = np.eye(2), np.eye(n)
    # unknowns [Ku_1, Ku_2, Kv_1, Kv_2]
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


def transform(scheme):
    """(lambda, tau, sigma, mu) from numpy's eigen-decomposition of A_rk, lambda the eigenvalue with positive imaginary part
    first.  Only the products mu tau_i and mu sigma are independent of the eigenvector's scaling."""
    Ark, b, _ = BUTCHER[scheme]
    w, T = np.linalg.eig(Ark)
    if w[0].imag < 0:
        w, T = w[::-1], T[:, ::-1]
    tau = np.linalg.inv(T)[0]
    return w[0], tau, tau[0] + tau[1], b @ T[:, 0]


def heat_one_solve(A, M, scheme, dt, n_steps, u0, loads=None):
    """The one-solve form of the issue, numpy complex128, the step matrix solved densely."""
    lam, tau, _, mu = transform(scheme)
    z = dt * lam
    S = M + z * A
    u, out = np.array(u0, dtype=np.float64), [np.array(u0, dtype=np.float64)]
    for k in range(n_steps):
        g = A @ u
        r = tau[0] * (_load(loads, k, 0, u.shape) - g) + tau[1] * (_load(loads, k, 1, u.shape) - g)
        w = np.linalg.solve(S, r)
        u = u + 2.0 * dt * (mu * w).real
        out.append(u)
    return np.array(out)


def wave_one_solve(A, M, scheme, dt, n_steps, u0, v0, dm=0.0, ds=0.0, loads=None):
    lam, tau, sigma, mu = transform(scheme)
    z = dt * lam
    S = (1.0 + z * dm) * M + (z * ds + z * z) * A
    u, v = np.array(u0, dtype=np.float64), np.array(v0, dtype=np.float64)
    us, vs = [u], [v]
    for k in range(n_steps):
        r = tau[0] * _load(loads, k, 0, u.shape) + tau[1] * _load(loads, k, 1, u.shape) \
            - sigma * (A @ (u + (z + ds) * v) + dm * (M @ v))
        wv = np.linalg.solve(S, r)
        wu = sigma * v + z * wv
        u, v = u + 2.0 * dt * (mu * wu).real, v + 2.0 * dt * (mu * wv).real
        us.append(u), vs.append(v)
    return np.array(us), np.array(vs)


def growth(A, M, scheme, order, dt, dm=0.0, ds=0.0, perm=None):
    """(growth, yardstick) of the unpivoted complex LDL^T of the step matrix in factor order."""
    S = step_matrix(A, M, scheme, order, dt, dm, ds)
    if perm is not None:
        S = S[np.ix_(perm, perm)]
    ref = zldl_reference(S)
    assert ref.bad < 0, ("bad pivot", ref.bad)
    return ref.G / ref.norm, ref


def stage_loads(rng, n_steps, shape):
    return rng.standard_normal((2 * n_steps,) + tuple(shape))


# ---- the surrogate pencil with its spectrum (CPU), and the four GPU cases with theirs

_q1 = {}


def q1_case(inner=7, contrast=1e4):
    """(A, M, lam, X) of the Q1 surrogate, X^T M X = I; built once."""
    import scipy.linalg as sl
    key = (inner, contrast)
    if key not in _q1:
        A, M = q1_pencil(inner, contrast)
        lam, X = sl.eigh(A, M)
        _q1[key] = (A, M, lam, X)
    return _q1[key]


def irk_case(so, name):
    """lod_harmonic_cases.harmonic_case(name): .A, .M, .lam_h, .X, .perm, .sym, .mvalues, .cols, .g; built once there."""
    from lod_harmonic_cases import harmonic_case
    return harmonic_case(so, name)
