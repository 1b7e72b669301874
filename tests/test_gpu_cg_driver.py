"""GPU tests of what the scalar-CG driver (csrc/slod_cg.hip.h) does around the steps of a solver and that
no other test pins: the iteration count when the cap is no multiple of the burst length (8 for
slod_lod_solve, 4 for the multigrid-preconditioned FEM solve, 32 for its Jacobi branch), the degenerate
solves (no iteration allowed, zero right-hand side), and the row-id check of the rows[] uploader with its
error texts.  H = 1/8, n = 4, l = 1: 64 patches, a 33^2 fine grid (multigrid levels 32/16/8/4/2) and a
9^2 coarse grid (levels 8/4/2)."""
import numpy as np
import pytest

from conftest import SEED, make_fields
from lod_cases import _lod_matrix, _mk, _torch, _upload

pytestmark = pytest.mark.gpu

SLOD_ERR_ARGUMENT = -1
_cache = {}


def _system(so, s):
    """Handle, basis, A_LOD block rows and the load vectors for spacedim s; built once per session."""
    if s not in _cache:
        torch, dev = _torch()
        cfg, g = _mk(so, nref=3, n_sub=4, oversampling=1, spacedim=s, stabilize=1)
        _upload(g, make_fields(so, cfg, "D100"))
        ids = np.arange(g.num_patches, dtype=np.uint32)
        plan = g.plan(ids)
        b = torch.zeros(len(ids) * plan.stride, dtype=torch.float64, device=dev)
        q = torch.zeros_like(b)
        plan.execute(b.data_ptr(), q.data_ptr())
        plan.status()
        values, cols = _lod_matrix(g, b, q, plan.stride, s)
        fine_rhs = torch.zeros((g.NE + 1) ** 2 * s, dtype=torch.float64, device=dev)
        g.fem_rhs(None, fine_rhs.data_ptr())
        lod_rhs = torch.zeros(g.num_patches * s, dtype=torch.float64, device=dev)
        g.lod_rhs(ids, b.data_ptr(), plan.stride, fine_rhs.data_ptr(), lod_rhs.data_ptr())
        # The 2-norm of a CG residual need not fall: for the smooth load f = 1 Jacobi-CG raises it above ||b||
        # over the first ten steps (2.19 at step 5 for spacedim 1).  The Jacobi cases take a rough load, whose
        # residual falls from the first step (0.16 / 0.0035 at steps 5 / 33 in a numpy model of the same
        # recurrence, 0.31 / 0.016 for spacedim 2), so that the (0, 1) check below says something about them.
        rough = np.random.default_rng(SEED).uniform(-1.0, 1.0, fine_rhs.numel())
        rough_rhs = torch.from_numpy(rough).to(dev)
        coarse_rhs = torch.zeros((g.N + 1) ** 2 * s, dtype=torch.float64, device=dev)
        g.coarse_fem_rhs(None, coarse_rhs.data_ptr())
        torch.cuda.synchronize()
        _cache[s] = dict(g=g, stride=plan.stride, basis=b, premult=q, values=values, cols=cols, fine_rhs=fine_rhs,
                         rough_rhs=rough_rhs, lod_rhs=lod_rhs, coarse_rhs=coarse_rhs)
    return _cache[s]


def _solve(S, solver, rhs, rel_tol, max_iterations):
    """One solve on a copy of u that starts as garbage: returns (iterations, residual, u)."""
    torch, _ = _torch()
    u = torch.full_like(rhs, 7.0)
    g = S["g"]
    if solver == "lod":
        it, res = g.lod_solve(S["values"].data_ptr(), S["cols"].data_ptr(), rhs.data_ptr(), u.data_ptr(), rel_tol,
                              max_iterations)
    elif solver == "coarse":
        it, res = g.coarse_fem_solve(rhs.data_ptr(), u.data_ptr(), rel_tol, max_iterations)
    else:
        it, res = g.fem_solve(rhs.data_ptr(), u.data_ptr(), rel_tol, max_iterations)
    torch.cuda.synchronize()
    return it, res, u


# (solver, SLOD_FEM_PRECOND, spacedim, name of the right-hand side)
SOLVERS = {"lod": ("lod", None, 1, "lod_rhs"),
           "fem_mg": ("fem", None, 1, "fine_rhs"),
           "fem_jacobi": ("fem", "jacobi", 1, "rough_rhs"),
           "fem_jacobi_2": ("fem", "jacobi", 2, "rough_rhs"),
           "coarse": ("coarse", None, 1, "coarse_rhs")}


def _case(so, monkeypatch, name):
    solver, precond, s, rhs = SOLVERS[name]
    if precond:
        monkeypatch.setenv("SLOD_FEM_PRECOND", precond)
    else:
        monkeypatch.delenv("SLOD_FEM_PRECOND", raising=False)
    S = _system(so, s)
    return S, solver, S[rhs]


@pytest.mark.parametrize("name,cap", [("lod", 3), ("lod", 9), ("fem_mg", 1), ("fem_mg", 5), ("fem_jacobi", 5),
                                      ("fem_jacobi", 33), ("fem_jacobi_2", 5), ("fem_jacobi_2", 33), ("coarse", 5)])
def test_cap_that_is_no_multiple_of_the_burst(so, monkeypatch, name, cap):
    """rel_tol = 0 never converges: the solver runs exactly max_iterations steps, the last burst cut short,
    and reports the residual of the last step."""
    S, solver, rhs = _case(so, monkeypatch, name)
    it, res, u = _solve(S, solver, rhs, 0.0, cap)
    print("%s cap %d: %d iterations, residual %.3e" % (name, cap, it, res))
    assert it == cap
    assert np.isfinite(res) and 0.0 < res < 1.0
    assert bool(u.isfinite().all())


@pytest.mark.parametrize("name", list(SOLVERS))
def test_no_iteration_allowed(so, monkeypatch, name):
    """max_iterations = 0: the init kernels run (u = 0), no step does; the residual is that of u = 0."""
    S, solver, rhs = _case(so, monkeypatch, name)
    it, res, u = _solve(S, solver, rhs, 1e-12, 0)
    assert it == 0 and res == 1.0
    assert float(u.abs().max()) == 0.0


@pytest.mark.parametrize("name", list(SOLVERS))
def test_zero_right_hand_side(so, monkeypatch, name):
    torch, _ = _torch()
    S, solver, rhs = _case(so, monkeypatch, name)
    it, res, u = _solve(S, solver, torch.zeros_like(rhs), 1e-12, 7)
    assert it == 0 and res == 0.0
    assert float(u.abs().max()) == 0.0


def _row_calls(S):
    """The four entry points that take a host rows[] array, as callables of rows."""
    torch, dev = _torch()
    g, s, b, q, st = S["g"], S["g"].spacedim, S["basis"], S["premult"], S["stride"]
    cap, n_rhs, ld = g.lod_row_capacity(), 3, S["fine_rhs"].numel()
    values = torch.zeros(g.num_patches * cap * s * s, dtype=torch.float64, device=dev)
    cols = torch.zeros(g.num_patches * cap, dtype=torch.int32, device=dev)
    out = torch.zeros(g.num_patches * s * n_rhs, dtype=torch.float64, device=dev)
    fine = S["fine_rhs"].repeat(n_rhs)
    return {
        "slod_lod_matrix": lambda rows: g.lod_matrix(rows, b.data_ptr(), q.data_ptr(), st, values.data_ptr(), cols.data_ptr()),
        "slod_lod_rhs": lambda rows: g.lod_rhs(rows, b.data_ptr(), st, S["fine_rhs"].data_ptr(), out.data_ptr()),
        "slod_lod_rhs_multi": lambda rows: g.lod_rhs_multi(rows, b.data_ptr(), st, fine.data_ptr(), ld, n_rhs, out.data_ptr(),
                                                           n_rhs),
        "slod_lod_mass_matrix": lambda rows: g.lod_mass_matrix(rows, b.data_ptr(), st, values.data_ptr(), cols.data_ptr()),
    }


ROW_TEXT = {"slod_lod_matrix": "row patch id out of range",
            "slod_lod_rhs": "row patch id out of range",
            "slod_lod_rhs_multi": "row patch id out of range",
            "slod_lod_mass_matrix": "slod_lod_mass_matrix: row patch id out of range"}


@pytest.mark.parametrize("entry", list(ROW_TEXT))
def test_row_id_out_of_range(so, entry):
    import slod_amd
    S = _system(so, 1)
    g = S["g"]
    with pytest.raises(slod_amd.SlodError) as err:
        _row_calls(S)[entry](np.array([0, g.num_patches], dtype=np.uint32))
    assert err.value.code == SLOD_ERR_ARGUMENT
    assert str(err.value) == "slod error %d: %s" % (SLOD_ERR_ARGUMENT, ROW_TEXT[entry])


@pytest.mark.parametrize("entry", list(ROW_TEXT))
def test_no_rows(so, entry):
    """n_rows = 0 is SLOD_OK (the wrapper raises on anything else)."""
    _row_calls(_system(so, 1))[entry](np.zeros(0, dtype=np.uint32))
