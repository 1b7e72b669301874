"""GPU tests of the multigrid V-cycle of the FEM reference solves (csrc/slod_fem.hip: k_mg_galerkin, k_mg_rowsum,
k_mg_smooth, k_mg_restrict, k_mg_prolong_add, MgHierarchy, and k_pcg_init / k_pcg_dot_rz / k_pcg_update_xr around
it) against the sparse restatement of tests/mg_cases.py, through slod_fem_solve and slod_coarse_fem_solve alone.

With rel_tol = 0 and max_iterations = 1 a solve returns u_1 = alpha B f, alpha = f.Bf / (Bf . A Bf): the V-cycle B
applied to the load, up to a scale that cancels as it does in PCG.  Unit loads read B column by column, dense loads fix
the scale between the columns, max_iterations 2, 3, 5, 8 follow the PCG recurrences across a burst of 4, and the
iteration count pins the stop test.  Bars: max(1e-13, 100 e64) relative to max |reference| (mg_cases.py); NE = 16 has
no longdouble reference and takes the largest e64 of the smaller grids."""
import numpy as np
import pytest

import mg_cases as mg
from conftest import make_fields
from lod_cases import _mk, _torch, _upload

pytestmark = pytest.mark.gpu

ids = mg.case_id
_handles = {}


def _handle(so, case):
    """The handle of a case with its coefficient uploaded; for a coarse case the sampled field the reference matrix was
    built from is what slod_coarse_coefficient returns, bit for bit."""
    if case not in _handles:
        torch, dev = _torch()
        _, g = _mk(so, **mg.case_kw(case))
        fine, solved = mg.fields_of(so, case)
        _upload(g, fine)
        if case[0] == "coarse":
            for f in range(case[2]):
                out = torch.zeros(g.N * g.N * 4, dtype=torch.float64, device=dev)
                g.coarse_coefficient(f, out.data_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy(), solved[f])
        assert (g.NE if case[0] == "fine" else g.N) == case[1]
        _handles[case] = g
    return _handles[case]


def _precond(monkeypatch, case, name=None):
    """Scalar problems take the V-cycle by default; vector problems are asked for it."""
    if name is None and case[2] == 1:
        monkeypatch.delenv("SLOD_FEM_PRECOND", raising=False)
    else:
        monkeypatch.setenv("SLOD_FEM_PRECOND", name or "mg")


def _solve_many(so, case, F, rel_tol, max_iterations):
    """One solve per column of F (loads on the interior dofs).  Returns (iterations, residuals, U on the interior dofs
    [n][k], the largest |u| on a rim dof)."""
    torch, dev = _torch()
    g = _handle(so, case)
    _, idx = mg.problem(so, case)
    ntot = (case[1] + 1) ** 2 * case[2]
    full = np.zeros((F.shape[1], ntot))
    full[:, idx] = F.T
    dF = torch.from_numpy(full).to(dev)
    dU = torch.full_like(dF, 7.0)            # every word must be written
    solver = g.fem_solve if case[0] == "fine" else g.coarse_fem_solve
    its, ress = [], []
    for j in range(F.shape[1]):
        it, res = solver(dF[j].data_ptr(), dU[j].data_ptr(), rel_tol, max_iterations)
        its.append(it), ress.append(res)
    torch.cuda.synchronize()
    U = dU.cpu().numpy()
    rim = np.ones(ntot, bool)
    rim[idx] = False
    return its, ress, U[:, idx].T, float(np.abs(U[:, rim]).max())


def _bars(so, case, e64, what):
    if e64 is None:
        e64 = mg.largest_small_e64(so, what)
    return mg.bar(e64)


def compare_u1(so, case, omega="rule"):
    """Shares of the bar the device uses on u_1, per unit load and per dense load, and a text per load over the bar."""
    A, _ = mg.problem(so, case)
    ref = mg.reference_u1(so, case, omega)
    dofs = mg.unit_load_dofs(so, case)
    E = np.zeros((A.shape[0], dofs.size))
    E[dofs, np.arange(dofs.size)] = 1.0
    out, bad = {}, []
    for name, F, want, e64 in (("unit", E, ref["unit"], ref["e64_unit"]), ("dense", mg.dense_loads(so, case), ref["dense"], ref["e64_dense"])):
        its, _, U, rim = _solve_many(so, case, F, 0.0, 1)
        assert its == [1] * F.shape[1]
        assert rim == 0.0, "%s %s loads: |u| = %.3e on the rim" % (ids(case), name, rim)
        share = mg.rel_dist(U, want) / _bars(so, case, e64, "u1")
        out[name] = share
        for j in np.nonzero(~(share <= 1.0))[0]:
            where = mg.describe_dof(case, dofs[j]) if name == "unit" else "dense load %d" % j
            worst = int(np.abs(U[:, j] - want[:, j]).argmax())
            bad.append("%s: %.2e bars; the largest deviation is at %s" % (where, share[j], mg.describe_dof(case, worst)))
    return out, bad


def compare_trajectory(so, case, omega="rule"):
    """{k: share of the bar} of u_k on dense load 0."""
    ref, e64 = mg.reference_trajectory(so, case, omega)
    f = mg.dense_loads(so, case)[:, :1]
    out = {}
    for k in mg.TRAJECTORY_STEPS:
        its, _, U, rim = _solve_many(so, case, f, 0.0, k)
        assert its == [k] and rim == 0.0
        out[k] = float(mg.rel_dist(U, ref[k][:, None])[0] / _bars(so, case, None if e64 is None else e64[k], "traj"))
    return out


@pytest.mark.parametrize("case", mg.CASES, ids=ids)
def test_first_step_is_the_reference_v_cycle(so, monkeypatch, case):
    _precond(monkeypatch, case)
    share, bad = compare_u1(so, case)
    print("PARITY %s u_1: largest share of the bar %.3f over %d unit loads, %.3f over %d dense loads"
          % (ids(case), share["unit"].max(), share["unit"].size, share["dense"].max(), share["dense"].size))
    assert not bad, "%s, %d loads over the bar:\n  %s" % (ids(case), len(bad), "\n  ".join(bad[:12]))


@pytest.mark.parametrize("case", mg.CASES, ids=ids)
def test_trajectory_is_the_reference_pcg(so, monkeypatch, case):
    _precond(monkeypatch, case)
    share = compare_trajectory(so, case)
    print("PARITY %s u_k: share of the bar %s" % (ids(case), ", ".join("k=%d %.3f" % kv for kv in share.items())))
    assert max(share.values()) <= 1.0, share


@pytest.mark.parametrize("case", mg.CASES, ids=ids)
def test_iteration_count_is_the_reference_burst(so, monkeypatch, case):
    """The stop test once per burst of 4: the count at rel_tol = tol is the reference's first multiple of 4 under tol
    (tol keeps a factor 10 from every burst end of the reference: test_mg_reference.py)."""
    _precond(monkeypatch, case)
    f, tol, expected, ends = mg.count_case(so, case)
    its, ress, _, rim = _solve_many(so, case, f[:, None], tol, 1000)
    print("%s: tol %.0e, %d iterations (reference %d), residual %.2e (reference %.2e)"
          % (ids(case), tol, its[0], expected, ress[0], ends[expected // mg.BURST - 1]))
    assert its[0] == expected and ress[0] <= tol and rim == 0.0


@pytest.mark.parametrize("N,s", [(5, 1), (5, 2), (2, 1), (2, 2)])
def test_grids_without_a_hierarchy_take_jacobi(so, monkeypatch, N, s):
    """NE odd or below 4: a solve that asks for the V-cycle is the Jacobi solve -- the same count, and u within 1e-12
    of max |u| (the atomic sums are unordered, the words need not be equal).  Through the coarse solve, whose grid is
    the N x N coarse cells."""
    torch, dev = _torch()
    cfg, g = _mk(so, n_cells=N, n_sub=4, oversampling=1, spacedim=s, stabilize=1)
    _upload(g, make_fields(so, cfg, "D1e4"))
    rhs = torch.zeros((N + 1) ** 2 * s, dtype=torch.float64, device=dev)
    g.coarse_fem_rhs(None, rhs.data_ptr())
    got = {}
    for name in ("mg", "jacobi"):
        monkeypatch.setenv("SLOD_FEM_PRECOND", name)
        u = torch.full_like(rhs, 7.0)
        it, res = g.coarse_fem_solve(rhs.data_ptr(), u.data_ptr(), 1e-12, 1000)
        torch.cuda.synchronize()
        got[name] = (it, res, u.cpu().numpy())
    print("N %d, s %d: mg %d iterations, jacobi %d" % (N, s, got["mg"][0], got["jacobi"][0]))
    assert got["mg"][0] == got["jacobi"][0] > 0 and got["mg"][1] <= 1e-12
    assert np.abs(got["mg"][2] - got["jacobi"][2]).max() <= 1e-12 * np.abs(got["jacobi"][2]).max()
