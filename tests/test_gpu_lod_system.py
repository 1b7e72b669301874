"""GPU tests of the rows SURVEY 8(f) marks "next": the global LOD system built from (phi, psi) --
A_LOD = C^T (A C) and C^T f (reference assemble_global_matrix LOD.cc:860-973, solve LOD.cc:976-1002),
its solve, the fine-scale reconstruction (LOD.cc:1251) -- and the inputs of the path produced on
the device (patch descriptors, coefficient sampling).  Reference-held numbers used:
  tests/parallel_assembly.output   all-ones basis, 32 x 32 A_LOD, exact integers
  tests/Poisson_LOD_Example.output  "fem rhs l2 norm = 0.109375" (exact), "rhs l2 norm = 0.0808367"
                                    (depends on the unseeded rand() stream: statistical, ~1e-2)
  tests/create_patch_01.output      patch sizes in Morton order
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_fields
from lod_cases import _fem_reference, _global_dense, _lod_matrix, _mk, _rows_to_dense, _torch, _upload
from mg_cases import PREDICTED_65

pytestmark = pytest.mark.gpu


def test_parallel_assembly_golden(so):
    """tests/parallel_assembly.cc: H=1/4, n=2, l=1, LOD<2,2>, every basis function == 1 on its patch
    (premultiplied too): A_LOD[(p,d),(q,e)] = 2 * #shared fine nodes.  The 1024 printed entries
    come out of the HIP kernel exactly."""
    torch, dev = _torch()
    cfg, g = _mk(so, nref=2, n_sub=2, oversampling=1, spacedim=2, stabilize=1)
    s = 2
    plan = g.plan(np.arange(g.num_patches, dtype=np.uint32))   # only for the slab stride
    stride = plan.stride
    hb = np.zeros(g.num_patches * stride)
    for p in range(g.num_patches):
        info = g.patch_layout(p)
        hb[p * stride:p * stride + s * info.n_fine] = 1.0
    b = torch.from_numpy(hb).to(dev)
    values, cols = _lod_matrix(g, b, b, stride, s)
    A = _rows_to_dense(g, values.cpu().numpy(), cols.cpu().numpy().view(np.uint32), s)
    lines = open(os.path.join(GOLDEN, "reference", "parallel_assembly.output")).read().split("\n")
    n = 0
    for ln in lines:
        if not ln.startswith("("):
            continue
        ij, val = ln.split(")")
        i, j = (int(x) for x in ij[1:].split(","))
        assert A[i, j] == float(val), (i, j, A[i, j], val)
        n += 1
    assert n == 1024
    # the pattern entry point agrees with the kernel's columns
    c = cols.cpu().numpy().view(np.uint32).reshape(g.num_patches, -1)
    for p in range(g.num_patches):
        assert sorted(int(x) for x in c[p] if x != 0xffffffff) == g.lod_pattern(p)


@pytest.mark.parametrize("kw", [dict(nref=3, n_sub=4, oversampling=1, spacedim=1),
                                dict(nref=3, n_sub=2, oversampling=2, spacedim=1),
                                dict(nref=2, n_sub=4, oversampling=1, spacedim=2)])
def test_lod_system_matches_dense_numpy(so, kw):
    """A_LOD, C^T f, the coarse solve and the reconstruction from the HIP kernels against dense
    numpy on the same (phi, psi): A = Phi Psi^T over the global fine grid, u = A^-1 C^T f,
    u_fine = Phi^T u."""
    torch, dev = _torch()
    cfg, g = _mk(so, stabilize=1, **kw)
    s = kw["spacedim"]
    fields = make_fields(so, cfg, "D100")
    _upload(g, fields)
    ids = np.arange(g.num_patches, dtype=np.uint32)
    plan = g.plan(ids)
    stride = plan.stride
    b = torch.zeros(len(ids) * stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    values, cols = _lod_matrix(g, b, q, stride, s)
    A = _rows_to_dense(g, values.cpu().numpy(), cols.cpu().numpy().view(np.uint32), s)
    Phi, Psi = _global_dense(g, s, b.cpu().numpy(), q.cpu().numpy(), stride)
    Aref = Phi @ Psi.T
    scale = np.abs(Aref).max()
    assert np.abs(A - Aref).max() <= 1e-12 * scale
    assert np.abs(A - A.T).max() <= 1e-9 * scale          # A_LOD is symmetric up to the basis accuracy
    # rhs: f = 1 lumped on the interior fine nodes (the "fem rhs" of Poisson_LOD_Example for f == 1)
    NEp = g.NE + 1
    hfine = 1.0 / g.NE
    f = np.zeros((NEp, NEp, s))
    f[1:-1, 1:-1, :] = hfine * hfine
    ft = torch.from_numpy(f.ravel()).to(dev)
    rhs = torch.zeros(g.num_patches * s, dtype=torch.float64, device=dev)
    g.lod_rhs(ids, b.data_ptr(), stride, ft.data_ptr(), rhs.data_ptr())
    torch.cuda.synchronize()
    rref = Phi @ f.ravel()
    assert np.abs(rhs.cpu().numpy() - rref).max() <= 1e-13 * np.abs(rref).max()
    # coarse solve (Jacobi-CG on the device) vs a dense solve, then u_fine = C u_H
    u = torch.zeros_like(rhs)
    it, res = g.lod_solve(values.data_ptr(), cols.data_ptr(), rhs.data_ptr(), u.data_ptr(), 1e-13, 5000)
    uref = np.linalg.solve(0.5 * (Aref + Aref.T), rref)
    assert res <= 1e-12 and it > 0
    assert np.abs(u.cpu().numpy() - uref).max() <= 1e-8 * np.abs(uref).max()
    fine = torch.zeros(NEp * NEp * s, dtype=torch.float64, device=dev)
    g.lod_reconstruct(b.data_ptr(), stride, u.data_ptr(), fine.data_ptr())
    torch.cuda.synchronize()
    fref = Phi.T @ u.cpu().numpy()
    assert np.abs(fine.cpu().numpy() - fref).max() <= 1e-12 * np.abs(fref).max()


def test_poisson_lod_example_rhs_norm(so):
    """tests/Poisson_LOD_Example.output: H=1/4, n=2, l=1, plain LOD, constant_coefficients (matrix
    re-use quirk) with a rand() field Alpha(1,100,8), f == 1.  'fem rhs l2 norm = 0.109375' is exact;
    'rhs l2 norm = 0.0808367' depends on the unseeded rand() stream at capture time: the whole HIP
    chain (assemble, solve, LOD selection, normalise, C^T f) reproduces it to the 1e-2 level the
    golden can pin (seeds give 0.0803 .. 0.0811)."""
    torch, dev = _torch()
    cfg, g = _mk(so, nref=2, n_sub=2, oversampling=1, stabilize=0, reuse_full=1)
    field = so.fill_coefficient_rand(1.0, 100.0, 8, g.NE, seed=1)
    g.set_coefficient(0, field)
    ids = np.arange(g.num_patches, dtype=np.uint32)
    plan = g.plan(ids)
    b = torch.zeros(len(ids) * plan.stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    NEp = g.NE + 1
    f = np.zeros((NEp, NEp))
    f[1:-1, 1:-1] = (1.0 / g.NE) ** 2
    assert abs(np.linalg.norm(f) - 0.109375) < 1e-15
    ft = torch.from_numpy(f.ravel()).to(dev)
    rhs = torch.zeros(g.num_patches, dtype=torch.float64, device=dev)
    g.lod_rhs(ids, b.data_ptr(), plan.stride, ft.data_ptr(), rhs.data_ptr())
    torch.cuda.synchronize()
    nrm = float(torch.linalg.norm(rhs))
    assert abs(nrm - 0.0808367) < 1e-3, nrm


def test_device_patch_layout_matches_host_and_golden():
    """Patch descriptors from the device kernel == the host index calculus, and both reproduce
    tests/create_patch_01.output (32 x 32 cells, oversampling 4, Morton order)."""
    import slod_amd
    g = slod_amd.Slod(nref=5, n_sub=1, oversampling=4)
    ids = np.arange(g.num_patches, dtype=np.uint32)
    dev_infos = g.device_patch_layout(ids)
    lines = open(os.path.join(GOLDEN, "reference", "create_patch_01.output")).read().strip().split("\n")[1:]
    for ln in lines:
        pid = int(ln.split(":")[0][2:])
        cnt = int(ln.split("{")[1].split("}")[0])
        assert dev_infos[pid].mx * dev_infos[pid].my == cnt
    # (reuse_full: under quirk Q1 the descriptors of all full patches carry the first one's coefficient origin;
    # the layout reported is the patch's own all the same)
    for kw in (dict(nref=3, n_sub=4, oversampling=2, spacedim=2), dict(n_cells=6, n_sub=3, oversampling=1), dict(nref=2, n_sub=2, oversampling=2, stabilize=0),
               dict(nref=3, n_sub=4, oversampling=1, reuse_full=1)):
        g = slod_amd.Slod(**kw)
        ids = np.arange(g.num_patches, dtype=np.uint32)
        for pid, di in zip(ids, g.device_patch_layout(ids)):
            hi = g.patch_layout(int(pid))
            assert bytes(di) == bytes(hi), (kw, pid)


def test_plan_descriptors_are_device_built_and_match_golden():
    """The descriptors a plan LAUNCHES with (slod_plan_patch_layout: read back from the device, where
    k_make_desc built them) reproduce tests/create_patch_01.output (32 x 32 cells, oversampling 4,
    Morton order) and the host index calculus; the balanced launch order is a permutation of the
    caller's list with non-increasing cost along the rank order; bad ids are rejected by the kernel."""
    import slod_amd
    # golden geometry (oversampling 4: 81 coarse dofs, beyond what the kernels run, so no plan): the
    # descriptor kernel k_make_desc through slod_device_patch_layout
    g = slod_amd.Slod(nref=5, n_sub=2, oversampling=4)
    ids = np.arange(g.num_patches, dtype=np.uint32)
    dinfo = g.device_patch_layout(ids)
    lines = open(os.path.join(GOLDEN, "reference", "create_patch_01.output")).read().strip().split("\n")[1:]
    for ln in lines:
        pid = int(ln.split(":")[0][2:])
        cnt = int(ln.split("{")[1].split("}")[0])
        assert dinfo[pid].mx * dinfo[pid].my == cnt
    # the same 32 x 32 grid at oversampling 3 as a plan: what the kernels launch with
    g = slod_amd.Slod(nref=5, n_sub=2, oversampling=3)
    plan = g.plan(ids)
    dinfo = g.device_patch_layout(ids)
    for pid in ids:
        info, idx = plan.patch_layout(int(pid))
        assert bytes(info) == bytes(dinfo[pid]) == bytes(g.patch_layout(int(pid))) and idx == pid
    for kw in (dict(nref=3, n_sub=4, oversampling=2, spacedim=2), dict(n_cells=6, n_sub=3, oversampling=1),
               dict(nref=2, n_sub=2, oversampling=2, stabilize=0), dict(nref=3, n_sub=4, oversampling=1, reuse_full=1)):
        g2 = slod_amd.Slod(**kw)
        ids2 = np.arange(g2.num_patches, dtype=np.uint32)[::-1].copy()
        plan2 = g2.plan(ids2)
        seen = set()
        for k, pid in enumerate(ids2):
            info, idx = plan2.patch_layout(k)
            assert bytes(info) == bytes(g2.patch_layout(int(pid))), (kw, pid)
            assert idx == k
            linfo, lidx = plan2.patch_layout(k, launch_order=True)
            seen.add(lidx)
            assert bytes(linfo) == bytes(g2.patch_layout(int(ids2[lidx])))
        assert seen == set(range(len(ids2)))
    with pytest.raises(slod_amd.SlodError) as e:
        g.plan(np.array([0, g.num_patches], dtype=np.uint32))
    assert e.value.code == -1


def test_device_coefficient_sampling_matches_reference_formula(so):
    """problem_parameter::value (Diffusion.h:40-53) sampled on the device at the points of
    quadrature_fine == the oracle's host evaluation of the same glibc rand() field, bit for bit;
    the basis built from it equals the basis built from the uploaded host field."""
    torch, dev = _torch()
    cfg, g = _mk(so, nref=3, n_sub=4, oversampling=1, stabilize=1)
    r, lo, hi = 4, 1.0, 100.0
    libc = C.CDLL("libc.so.6")
    libc.srand(7)
    f32 = np.float32
    vals = np.array([lo + float(f32(libc.rand()) / f32(f32(2147483647) / f32(hi - lo))) for _ in range(4 ** r)])
    field = so.fill_coefficient_rand(lo, hi, r, g.NE, seed=7)
    vt = torch.from_numpy(vals).to(dev)
    g.sample_coefficient(0, vt.data_ptr(), r)
    ids = np.arange(g.num_patches, dtype=np.uint32)
    b1, p1, _ = g.compute_basis(ids)
    g.set_coefficient(0, field)
    b0, p0, _ = g.compute_basis(ids)
    assert np.array_equal(b0, b1) and np.array_equal(p0, p1)


@pytest.mark.parametrize("n_pieces", [1, 3])
def test_execute_allgather_single_rank(so, n_pieces):
    """The C-ABI exchange path (slod_comm_* over RCCL, slod_plan_execute_allgather: pieces computed on
    one stream, exchanged on another) on ONE rank: bit-identical to slod_plan_execute, and the
    plain slod_comm_allgather copies the slab.  (Multi-rank runs are the driver's 8-GPU bench.)"""
    import slod_amd
    torch, dev = _torch()
    cfg, g = _mk(so, nref=3, n_sub=4, oversampling=1, stabilize=1)
    fields = make_fields(so, cfg, "D100")
    _upload(g, fields)
    ids = np.arange(g.num_patches, dtype=np.uint32)
    plan = g.plan(ids)
    ppr = len(ids) + 3                       # a padded slab, as on ranks with fewer patches
    ref_b = torch.zeros(ppr * plan.stride, dtype=torch.float64, device=dev)
    ref_q = torch.zeros_like(ref_b)
    plan.execute(ref_b.data_ptr(), ref_q.data_ptr())
    plan.status()
    comm = slod_amd.Comm(slod_amd.Comm.unique_id(), 1, 0, 0)
    b = torch.zeros_like(ref_b)
    q = torch.zeros_like(ref_b)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    plan.execute_allgather(comm, b.data_ptr(), q.data_ptr(), ppr, n_pieces, s1.cuda_stream, s2.cuda_stream)
    torch.cuda.synchronize()
    plan.status()
    assert torch.equal(b, ref_b) and torch.equal(q, ref_q)
    out = torch.zeros_like(ref_b)
    comm.allgather(b.data_ptr(), out.data_ptr(), b.numel(), s1.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out, b)
    comm.close()


# ---- fine FEM reference problem (assemble_and_solve_fem_problem, LOD.cc:1004-1094)


def test_fem_rhs_matches_example_golden(so):
    """'fem rhs l2 norm = 0.109375' of tests/Poisson_LOD_Example.output (H=1/4, n=2, f == 1) from
    the device load-vector kernel, and a non-constant f against the numpy quadrature."""
    torch, dev = _torch()
    cfg, g = _mk(so, nref=2, n_sub=2, oversampling=1, stabilize=0)
    NEp = g.NE + 1
    rhs = torch.zeros(NEp * NEp, dtype=torch.float64, device=dev)
    g.fem_rhs(None, rhs.data_ptr())
    torch.cuda.synchronize()
    assert abs(float(torch.linalg.norm(rhs)) - 0.109375) < 1e-15
    r = rhs.cpu().numpy().reshape(NEp, NEp)
    assert np.all(r[0] == 0) and np.all(r[-1] == 0) and np.all(r[:, 0] == 0) and np.all(r[:, -1] == 0)
    rng = np.random.default_rng(3)
    fq = rng.uniform(-1.0, 2.0, g.NE * g.NE * 4)
    g.fem_rhs(torch.from_numpy(fq).to(dev).data_ptr(), rhs.data_ptr())
    torch.cuda.synchronize()
    _, fref, idx = _fem_reference(g.NE, 1, [np.ones(g.NE * g.NE * 4)], fq)
    assert np.abs(rhs.cpu().numpy()[idx] - fref).max() <= 1e-15


@pytest.mark.parametrize("kw,dist", [(dict(nref=3, n_sub=4, oversampling=1, spacedim=1), "D100"),
                                     (dict(nref=3, n_sub=4, oversampling=1, spacedim=1), "D1e4"),
                                     (dict(nref=2, n_sub=4, oversampling=1, spacedim=2), "D100")])
def test_fem_solve_matches_sparse_direct(so, kw, dist):
    """Matrix-free (multigrid-preconditioned) CG on the device stencil planes against scipy's sparse direct solve of the
    same fine problem (independent assembly from oracle/slod_numpy.element_matrix)."""
    import scipy.sparse.linalg as spl
    torch, dev = _torch()
    cfg, g = _mk(so, stabilize=1, **kw)
    s = kw["spacedim"]
    fields = make_fields(so, cfg, dist)
    _upload(g, fields)
    NEp = g.NE + 1
    rhs = torch.zeros(NEp * NEp * s, dtype=torch.float64, device=dev)
    u = torch.zeros_like(rhs)
    g.fem_rhs(None, rhs.data_ptr())
    it, res = g.fem_solve(rhs.data_ptr(), u.data_ptr(), 1e-13, 50000)
    assert 0 < it < 50000 and res <= 1e-12
    A, f, idx = _fem_reference(g.NE, s, fields)
    uref = spl.spsolve(A, f)
    uh = u.cpu().numpy()
    assert np.abs(uh[idx] - uref).max() <= 1e-8 * np.abs(uref).max()
    mask = np.ones(uh.size, bool)
    mask[idx] = False
    assert np.all(uh[mask] == 0.0)


@pytest.mark.parametrize("spacedim", [1, 2])
def test_fem_multigrid_preconditioner(so, spacedim, monkeypatch):
    """The fine FEM reference solve is CG with a geometric multigrid V-cycle (Galerkin coarse operators
    on the stencil planes; the reference uses CG + AMG, LOD.cc:1070-1075).  Same solution as the
    Jacobi-preconditioned CG (SLOD_FEM_PRECOND=jacobi), several times fewer iterations at contrast 1e4."""
    torch, dev = _torch()
    kw = dict(nref=4, n_sub=4, oversampling=1, spacedim=spacedim)
    cfg, g = _mk(so, stabilize=1, **kw)
    fields = make_fields(so, cfg, "D1e4")
    _upload(g, fields)
    NEp = g.NE + 1
    rhs = torch.zeros(NEp * NEp * spacedim, dtype=torch.float64, device=dev)
    g.fem_rhs(None, rhs.data_ptr())
    u_mg = torch.zeros_like(rhs)
    it_mg, res_mg = g.fem_solve(rhs.data_ptr(), u_mg.data_ptr(), 1e-12, 20000)
    monkeypatch.setenv("SLOD_FEM_PRECOND", "jacobi")
    u_j = torch.zeros_like(rhs)
    it_j, res_j = g.fem_solve(rhs.data_ptr(), u_j.data_ptr(), 1e-12, 20000)
    assert res_mg <= 1e-12 and res_j <= 1e-12
    assert float((u_mg - u_j).abs().max()) <= 1e-8 * float(u_j.abs().max())
    if spacedim == 1:
        assert 0 < it_mg < it_j / 3, (it_mg, it_j)
    else:   # vector problems keep Jacobi by default (the V-cycle is opt-in there: SLOD_FEM_PRECOND=mg)
        assert it_mg == it_j
        # asked for, the V-cycle reaches the same solution in fewer iterations: at most twice the share of Jacobi's
        # count that the CPU reference predicts for this grid (mg_cases.PREDICTED_65, pinned by test_mg_reference.py)
        monkeypatch.setenv("SLOD_FEM_PRECOND", "mg")
        u_v = torch.zeros_like(rhs)
        it_v, res_v = g.fem_solve(rhs.data_ptr(), u_v.data_ptr(), 1e-12, 20000)
        print("elasticity with SLOD_FEM_PRECOND=mg: %d iterations (reference %d), Jacobi-CG %d (reference %d)"
              % (it_v, PREDICTED_65["mg"], it_j, PREDICTED_65["jacobi"]))
        assert res_v <= 1e-12
        assert float((u_v - u_j).abs().max()) <= 1e-8 * float(u_j.abs().max())
        assert 0 < it_v < it_j and it_v <= 2.0 * PREDICTED_65["mg"] / PREDICTED_65["jacobi"] * it_j, (it_v, it_j)
    print("fine FEM solve, %d components, 65^2 nodes, contrast 1e4: multigrid-CG %d iterations, Jacobi-CG %d" % (spacedim, it_mg, it_j))


def test_lod_solution_converges_to_fem_with_oversampling(so):
    """compare_lod_with_fem (LOD.cc:1240-1378) in one number: the reconstructed SLOD solution against
    the fine FEM solution of the same rough coefficient; the error drops with the oversampling."""
    torch, dev = _torch()
    errs = []
    for ell in (1, 2):
        cfg, g = _mk(so, nref=3, n_sub=4, oversampling=ell, stabilize=1)
        fields = make_fields(so, cfg, "D100")
        _upload(g, fields)
        ids = np.arange(g.num_patches, dtype=np.uint32)
        plan = g.plan(ids)
        stride = plan.stride
        b = torch.zeros(len(ids) * stride, dtype=torch.float64, device=dev)
        q = torch.zeros_like(b)
        plan.execute(b.data_ptr(), q.data_ptr())
        plan.status()
        NEp = g.NE + 1
        f = torch.zeros(NEp * NEp, dtype=torch.float64, device=dev)
        g.fem_rhs(None, f.data_ptr())
        ufem = torch.zeros_like(f)
        it, res = g.fem_solve(f.data_ptr(), ufem.data_ptr(), 1e-12, 50000)
        assert res <= 1e-11
        values, cols = _lod_matrix(g, b, q, stride, 1)
        rhs = torch.zeros(g.num_patches, dtype=torch.float64, device=dev)
        g.lod_rhs(ids, b.data_ptr(), stride, f.data_ptr(), rhs.data_ptr())
        uH = torch.zeros_like(rhs)
        g.lod_solve(values.data_ptr(), cols.data_ptr(), rhs.data_ptr(), uH.data_ptr(), 1e-13, 5000)
        ulod = torch.zeros_like(f)
        g.lod_reconstruct(b.data_ptr(), stride, uH.data_ptr(), ulod.data_ptr())
        torch.cuda.synchronize()
        errs.append(float(torch.linalg.norm(ulod - ufem) / torch.linalg.norm(ufem)))
    assert errs[1] < errs[0] and errs[1] < 2e-2, errs
