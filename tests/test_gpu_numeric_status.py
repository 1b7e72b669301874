"""The failure path of the patch solve: SLOD_ERR_NUMERIC from every kernel family, and what a plan is worth afterwards.

Every patch-solve family (k_solve_tw, k_solve_mf, k_solve = coop, k_solve_nd) ORs a bit into the plan's status word
when a pivot is not positive; slod_plan_status / slod_compute_basis turn it into SLOD_ERR_NUMERIC (-5).  The contract
(include/slod.h, DESIGN.md "The failure path of the patch solve"): after -5 every output and diagnostic of that execute
is undefined, the plan and the handle stay usable, and the next execute on valid coefficients gives the results of a
fresh plan bit for bit.

Inputs (lod_cases._bad_fields): the D100 base field with a 2 x 2 block of fine cells set to -1 ("negative": the patch
matrix is indefinite, all arithmetic stays finite, every elimination is symmetric so by inertia a pivot is not
positive) or NaN ("nan"), or with a full patch's 3 x 3 coarse cells set to 0 ("zero": exact zero pivots, Inf, NaN).
The block sits inside one interior coarse cell; over the two block positions and the nine positions of that cell in a
3 x 3 patch its middle node falls on the first and last interior line, on both chains and on the meeting line of the
sweeps.  The first test (no GPU) checks on the oracle that these fields hit exactly the patches that hold a bad cell.

Bars: the status code is exact; a patch without a bad cell meets lod_cases._check_patch (1e-10) against the oracle on
the base field; a recovered execute is compared with a fresh plan on a fresh handle as 64-bit words.
"""
import re

import numpy as np
import pytest

from lod_cases import (BAD_CELL, ERR_NUMERIC, NUMERIC_CONFIGS, _BaseOracle, _bad_fields, _bits, _check_patch,
                       _internal_matrix, _mk, _patch_bits, _patches_with_cells, _run, _status_of, _torch, _upload)

gpu = pytest.mark.gpu
FAMILY = {"mf": "k_solve_mf<", "tw": "k_solve_tw<", "coop": "k_solve<", "nd": "k_solve_nd<"}
_LAUNCH = re.compile(r"\[slod\] (k_solve(?:_tw|_mf|_nd)?<)[0-9,]+>: (\d+) patches")
KNOBS = ("SLOD_SOLVE", "SLOD_FUSE_SELECT", "SLOD_TWISTED", "SLOD_BWD_KSPLIT", "SLOD_WORKSPACE_MB", "SLOD_FUSE_M",
         "SLOD_FUSE_ASSEMBLE", "SLOD_SVD_REGS", "SLOD_BALANCE")
# patches that hold a bad cell.  On the 4 x 4-cell elasticity grid the zeroed 3 x 3 cells reach into every patch:
# there is no "other" patch in that one case and the status test expects -5 from all 16
HIT = {("scalar", "negative"): 9, ("scalar", "nan"): 9, ("scalar", "zero"): 25,
       ("elasticity", "negative"): 9, ("elasticity", "nan"): 9, ("elasticity", "zero"): 16}


def _variant(name, problem, solve, **env):
    return pytest.param(problem, solve, env, id=name)


# the status sites: every family, and for tw the split selection launch, the column-tile backward sweep and (a coop
# knob, without effect on tw) SLOD_TWISTED=0; coop with one chain instead of two
STATUS_VARIANTS = [
    _variant("scalar-mf", "scalar", "mf"), _variant("scalar-tw", "scalar", "tw"),
    _variant("scalar-coop", "scalar", "coop"), _variant("scalar-nd", "scalar", "nd"),
    _variant("scalar-tw-split-select", "scalar", "tw", SLOD_FUSE_SELECT="0"),
    _variant("scalar-tw-twisted0", "scalar", "tw", SLOD_TWISTED="0"),
    _variant("scalar-tw-ksplit0", "scalar", "tw", SLOD_BWD_KSPLIT="0"),
    _variant("scalar-coop-twisted0", "scalar", "coop", SLOD_TWISTED="0"),
    _variant("elasticity-tw", "elasticity", "tw"), _variant("elasticity-mf", "elasticity", "mf"),
]
RECOVERY_VARIANTS = [
    _variant("scalar-mf", "scalar", "mf"), _variant("scalar-tw-fused", "scalar", "tw", SLOD_FUSE_SELECT="1"),
    _variant("scalar-tw-split", "scalar", "tw", SLOD_FUSE_SELECT="0"), _variant("scalar-coop", "scalar", "coop"),
    _variant("scalar-nd", "scalar", "nd"),
    _variant("elasticity-tw", "elasticity", "tw"), _variant("elasticity-mf", "elasticity", "mf"),
]
TW_MF = [_variant("scalar-tw", "scalar", "tw"), _variant("scalar-mf", "scalar", "mf"),
         _variant("elasticity-tw", "elasticity", "tw"), _variant("elasticity-mf", "elasticity", "mf")]
KINDS = ["negative", "nan", "zero"]
KIND_BLOCKS = [("negative", 0), ("negative", 1), ("nan", 0), ("nan", 1), ("zero", 0)]   # (zero has no block position)


def _setenv(monkeypatch, solve, env, debug=True):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SLOD_SOLVE", solve)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SLOD_DEBUG", "1" if debug else "0")


def _case(so, problem, kind, block=0):
    """(oracle on the base field, handle with the bad field set, bad fields, ids of the patches with a bad cell)"""
    ref = _BaseOracle(so, problem)
    kw = NUMERIC_CONFIGS[problem]
    _, g = _mk(so, **kw)
    fields, cells = _bad_fields(ref.base, kw, kind, block)
    _upload(g, fields)
    hit = _patches_with_cells(so, ref.cfg, cells)
    assert len(hit) == HIT[problem, kind] and g.num_patches == so.num_patches(ref.cfg)
    return ref, g, fields, hit


def _sync():
    _torch()[0].cuda.synchronize()


def _decisions_of(plan):
    return [(d.path, d.n_cut, d.n_dropped) for d in plan.diagnostics()]


def _order(g, reverse=True):
    ids = np.arange(g.num_patches, dtype=np.uint32)
    return ids[::-1].copy() if reverse else ids      # reversed: launch order and slab order are not the id order


_fresh_store = {}


def _fresh(so, problem, solve, env, reverse=True):
    """Slabs (as 64-bit words) and decisions of a fresh plan on a fresh handle with the base field, under the
    environment the caller has set (without SLOD_WORKSPACE_MB: one chunk); computed once per variant, checked
    against the oracle once, read-only."""
    key = (problem, solve, tuple(sorted((k, v) for k, v in env.items() if k != "SLOD_WORKSPACE_MB")), reverse)
    if key not in _fresh_store:
        ref = _BaseOracle(so, problem)
        _, g = _mk(so, **NUMERIC_CONFIGS[problem])
        _upload(g, ref.base)
        ids = _order(g, reverse)
        plan = g.plan(ids)
        b, q = _run(plan)
        _sync()
        assert _status_of(plan) == (0, "")
        hb, hq = b.cpu().numpy(), q.cpu().numpy()
        for k, pid in enumerate(ids):
            _check_patch(ref, ref.cfg, ref.base, int(pid), hb, hq, k * plan.stride, "fresh " + solve)
        c = (_bits(b), _bits(q), _decisions_of(plan))
        for a in c[:2]:
            a.setflags(write=False)
        _fresh_store[key] = c
        plan.close()
        g.close()
    return _fresh_store[key]


def _assert_recovered(so, ref, plan, ids, b, q, fresh, label):
    """status OK, slabs bit-identical to the fresh plan's (which met the oracle), decisions equal"""
    _sync()
    assert _status_of(plan) == (0, ""), label
    fb, fq, fdec = fresh
    wb, wq = _bits(b), _bits(q)
    for k, pid in enumerate(ids):
        n = ref.cfg.spacedim * so.patch_info(ref.cfg, int(pid)).n_f
        s0 = k * plan.stride
        assert np.array_equal(wb[s0:s0 + n], fb[s0:s0 + n]) and np.array_equal(wq[s0:s0 + n], fq[s0:s0 + n]), \
            "%s: patch %d differs from the fresh plan's" % (label, pid)
    assert np.array_equal(wb, fb) and np.array_equal(wq, fq), label      # the gaps too: untouched
    assert _decisions_of(plan) == fdec, label


# ---------------------------------------------------------------- the inputs, on the oracle (no GPU)
@pytest.mark.parametrize("kind,block", KIND_BLOCKS)
@pytest.mark.parametrize("problem", ["scalar", "elasticity"])
def test_bad_fields_hit_exactly_the_patches_with_the_bad_cell(so, problem, kind, block):
    """negative: the internal matrix of every patch with the bad cell has a negative eigenvalue (dense, from the
    oracle's stencil).  zero: it has a row of exact zeros.  nan: it holds NaN.  Every other patch: the oracle's
    (phi, psi) on the bad field are those on the base field bit for bit.  At least nine patches are hit and, but
    for the elasticity grid under "zero" (see HIT), at least one is not."""
    ref = _BaseOracle(so, problem)
    kw, cfg = NUMERIC_CONFIGS[problem], ref.cfg
    fields, cells = _bad_fields(ref.base, kw, kind, block)
    assert all(f.shape == b.shape for f, b in zip(fields, ref.base)) and len(fields) == cfg.spacedim
    changed = sum(int((np.asarray(f) != np.asarray(b)).sum()) for f, b in zip(fields, ref.base))
    assert changed == cfg.spacedim * 4 * (4 if kind != "zero" else 9 * kw["n_sub"] ** 2)
    hit = _patches_with_cells(so, cfg, cells)
    NP = so.num_patches(cfg)
    assert len(hit) == HIT[problem, kind] >= 9
    assert len(hit) < NP or (problem, kind) == ("elasticity", "zero")
    if kind != "zero":
        assert cells == {BAD_CELL[problem]}
        # the cell takes every position a 3 x 3 neighbourhood allows
        pos = {(BAD_CELL[problem][0] - so.patch_info(cfg, p).x0, BAD_CELL[problem][1] - so.patch_info(cfg, p).y0,
                so.patch_info(cfg, p).mx, so.patch_info(cfg, p).my) for p in hit}
        assert len(pos) == 9
        if problem == "scalar":
            assert pos == {(i, j, 3, 3) for i in range(3) for j in range(3)}
    for pid in range(NP):
        if pid in hit:
            A = _internal_matrix(so, cfg, fields, pid)
            assert A.shape[0] <= 121 * cfg.spacedim
            if kind == "negative":
                assert np.isfinite(A).all() and np.array_equal(A, A.T)
                assert np.linalg.eigvalsh(A)[0] < -1e-3, pid
            elif kind == "zero":
                assert (np.abs(A).sum(axis=1) == 0.0).any(), pid
            else:
                assert np.isnan(np.diag(A)).any(), pid
        else:
            phi, psi, _ = so.patch_basis(cfg, fields, pid)
            phi0, psi0, _ = ref.patch_basis(cfg, ref.base, pid)
            assert np.array_equal(phi.view(np.uint64), phi0.view(np.uint64)), pid
            assert np.array_equal(psi.view(np.uint64), psi0.view(np.uint64)), pid


# ---------------------------------------------------------------- 1, 2: the status of every patch on its own
def _status_per_patch(so, problem, solve, env, kind, block, monkeypatch, capfd):
    _setenv(monkeypatch, solve, env)
    ref, g, fields, hit = _case(so, problem, kind, block)
    label = "%s %s %s block %d" % (problem, solve, kind, block)
    failed_in = set()
    for pid in range(g.num_patches):
        plan = g.plan(np.array([pid], dtype=np.uint32))
        capfd.readouterr()
        b, q = _run(plan)
        _sync()
        code, msg = _status_of(plan)
        launched = {m[0] for m in _LAUNCH.findall(capfd.readouterr().err)}
        # A one-patch plan of a rim patch two cells wide has lines of s * 7 dofs.  For s = 2 the tw lane tile
        # (T = 2 for 14 dofs) is narrower than the band (2 s - 1 = 3) and the dispatcher hands a plan that asked
        # for tw to coop (slod_choose_solver); the patches three cells wide (22 dofs, T = 3) run tw
        info = g.patch_layout(pid)
        narrow = solve == "tw" and ref.cfg.spacedim == 2 and min(info.mx, info.my) == 2
        assert launched == {FAMILY["coop" if narrow else solve]}, "%s patch %d: launched %s" % (label, pid, sorted(launched))
        if pid in hit:
            assert code == ERR_NUMERIC, "%s patch %d holds the bad cell: status %d" % (label, pid, code)
            assert "patch solve" in msg
            failed_in |= launched
        else:
            assert (code, msg) == (0, ""), "%s patch %d holds no bad cell: %s" % (label, pid, msg)
            _check_patch(ref, ref.cfg, ref.base, pid, b.cpu().numpy(), q.cpu().numpy(), 0, label)
        plan.close()
    assert FAMILY[solve] in failed_in          # the family asked for has set the status word
    g.close()


@gpu
@pytest.mark.parametrize("block", [0, 1])
@pytest.mark.parametrize("problem,solve,env", STATUS_VARIANTS)
def test_negative_block_sets_the_status_of_exactly_its_patches(so, problem, solve, env, block, monkeypatch, capfd):
    """One single-patch plan per patch id on the "negative" field: -5 exactly from the patches that hold the bad
    cell, status OK and oracle parity from every other one; the launch log names the family that set the status."""
    _status_per_patch(so, problem, solve, env, "negative", block, monkeypatch, capfd)


@gpu
@pytest.mark.parametrize("kind,block", KIND_BLOCKS[2:])
@pytest.mark.parametrize("problem,solve,env", TW_MF)
def test_nan_and_zero_set_the_status_of_exactly_their_patches(so, problem, solve, env, kind, block, monkeypatch, capfd):
    """The same with a NaN block (the comparison !(piv > 0.0) must catch it) and with a singular patch matrix (an
    exact zero pivot, Inf, then NaN)."""
    _status_per_patch(so, problem, solve, env, kind, block, monkeypatch, capfd)


# ---------------------------------------------------------------- 3: the host-buffer wrapper
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("problem", ["scalar", "elasticity"])
def test_compute_basis_reports_numeric_and_the_handle_stays_usable(so, problem, kind, monkeypatch):
    import slod_amd
    for k in KNOBS + ("SLOD_SOLVE", "SLOD_DEBUG"):
        monkeypatch.delenv(k, raising=False)
    ref, g, fields, hit = _case(so, problem, kind)
    ids = np.arange(g.num_patches)
    with pytest.raises(slod_amd.SlodError) as e:
        g.compute_basis(ids)
    assert e.value.code == ERR_NUMERIC and "patch solve" in str(e.value)
    _upload(g, ref.base)
    basis, premult, offs = g.compute_basis(ids)
    for k, pid in enumerate(ids):
        _check_patch(ref, ref.cfg, ref.base, int(pid), basis, premult, int(offs[k]), "after " + kind)
    g.close()


# ---------------------------------------------------------------- 4, 8: recovery of a plan
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("problem,solve,env", RECOVERY_VARIANTS)
def test_plan_recovers_bit_for_bit_after_a_failed_execute(so, problem, solve, env, kind, monkeypatch):
    """One plan over all patches (reversed ids): execute on the bad field (-5), set the base field, execute the SAME
    plan: status OK, outputs and decisions those of a fresh plan on a fresh handle, bit for bit.
    Recorded, not asserted: how many patches without a bad cell the failed execute still got right."""
    _setenv(monkeypatch, solve, env, debug=False)
    fresh = _fresh(so, problem, solve, env)
    ref, g, fields, hit = _case(so, problem, kind)
    ids = _order(g)
    plan = g.plan(ids)
    b, q = _run(plan)
    _sync()
    code, msg = _status_of(plan)
    assert code == ERR_NUMERIC and "patch solve" in msg
    others = [k for k, pid in enumerate(ids) if int(pid) not in hit]
    same = 0
    for k in others:
        n = ref.cfg.spacedim * so.patch_info(ref.cfg, int(ids[k])).n_f
        s0 = k * plan.stride
        same += int(np.array_equal(_patch_bits(plan, b, k, n), fresh[0][s0:s0 + n]) and
                    np.array_equal(_patch_bits(plan, q, k, n), fresh[1][s0:s0 + n]))
    print("NUMERIC_LEFT %s %s %s: %d of %d patches without a bad cell are bit-identical to the clean run"
          % (problem, solve + "".join("," + k + "=" + v for k, v in env.items()), kind, same, len(others)))
    _upload(g, ref.base)
    b, q = _run(plan)
    _assert_recovered(so, ref, plan, ids, b, q, fresh, "%s %s after %s" % (problem, solve, kind))
    plan.close()
    g.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("problem", ["scalar", "elasticity"])
def test_plan_recovers_through_update_coefficient(so, problem, kind, monkeypatch):
    """The refresh route: after the failed execute the base field comes back through slod_update_coefficient; the
    dirty plan (a new plan) overwrites the flagged patches of the failed slab in place, then the full plan that had
    failed executes again.  Both give the fresh plan's bits."""
    _setenv(monkeypatch, "tw", {}, debug=False)
    torch, dev = _torch()
    fresh = _fresh(so, problem, "tw", {}, reverse=False)
    ref, g, fields, hit = _case(so, problem, kind)
    ids = _order(g, reverse=False)
    plan = g.plan(ids)
    b, q = _run(plan)
    _sync()
    assert _status_of(plan)[0] == ERR_NUMERIC
    dirty = torch.zeros(g.num_patches, dtype=torch.int32, device=dev)
    for f, a in enumerate(ref.base):
        g.update_coefficient(f, a, dirty.data_ptr())
    flagged = g.dirty_patches(dirty.data_ptr()).tolist()
    assert flagged == hit
    dplan = g.plan_dirty(dirty.data_ptr())
    assert dplan.stride == plan.stride and dplan.gids.tolist() == hit
    dplan.execute(b.data_ptr(), q.data_ptr())
    _sync()
    assert _status_of(dplan) == (0, "")
    wb, wq = _bits(b), _bits(q)
    for pid in hit:
        n = ref.cfg.spacedim * so.patch_info(ref.cfg, pid).n_f
        s0 = pid * plan.stride
        assert np.array_equal(wb[s0:s0 + n], fresh[0][s0:s0 + n]) and np.array_equal(wq[s0:s0 + n], fresh[1][s0:s0 + n]), pid
    b, q = _run(plan)
    _assert_recovered(so, ref, plan, ids, b, q, fresh, "%s update_coefficient after %s" % (problem, kind))
    dplan.close()
    plan.close()
    g.close()


# ---------------------------------------------------------------- 5: a plan that re-uses its workspace slots
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_chunked_plan_recovers(so, kind, monkeypatch, capfd):
    """SLOD_WORKSPACE_MB=1: 55 KB of workspace per patch, so the 64 patches run in at least three launches that
    re-use the slots (the launch log counts them).  A failing patch is in the first launch.  -5, then the bits of the
    fresh plan that ran in one chunk."""
    _setenv(monkeypatch, "tw", {}, debug=False)
    fresh = _fresh(so, "scalar", "tw", {})
    _setenv(monkeypatch, "tw", {"SLOD_WORKSPACE_MB": "1"})
    ref, g, fields, hit = _case(so, "scalar", kind)
    ids = _order(g)
    plan = g.plan(ids)
    capfd.readouterr()
    b, q = _run(plan)
    _sync()
    launches = _LAUNCH.findall(capfd.readouterr().err)
    assert len(launches) >= 3 and {m[0] for m in launches} == {FAMILY["tw"]}
    assert sum(int(m[1]) for m in launches) == len(ids)
    first = {int(ids[plan.patch_layout(k, launch_order=True)[1]]) for k in range(int(launches[0][1]))}
    assert first & set(hit), "no failing patch in the first chunk"
    assert _status_of(plan)[0] == ERR_NUMERIC
    _upload(g, ref.base)
    b, q = _run(plan)
    _assert_recovered(so, ref, plan, ids, b, q, fresh, "chunked after " + kind)
    plan.close()
    g.close()


# ---------------------------------------------------------------- 6: two workspaces
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_overlap_depth_2_recovers_in_the_poisoned_workspace(so, kind, monkeypatch):
    """set_overlap(2): the failed execute used workspace 0.  With the base field set, execute A (workspace 1) and
    execute B (workspace 0) run back to back; after the join the status is OK and both have the fresh plan's bits."""
    _setenv(monkeypatch, "tw", {}, debug=False)
    fresh = _fresh(so, "scalar", "tw", {})
    ref, g, fields, hit = _case(so, "scalar", kind)
    ids = _order(g)
    plan = g.plan(ids)
    plan.set_overlap(2)
    _run(plan)
    assert _status_of(plan)[0] == ERR_NUMERIC          # (synchronises the device)
    _upload(g, ref.base)
    ba, qa = _run(plan)
    bb, qb = _run(plan)
    plan.join()
    _assert_recovered(so, ref, plan, ids, bb, qb, fresh, "overlap B after " + kind)
    assert np.array_equal(_bits(ba), fresh[0]) and np.array_equal(_bits(qa), fresh[1])
    plan.close()
    g.close()


@gpu
def test_overlap_depth_2_status_covers_the_last_execute_of_each_workspace(so, monkeypatch):
    """slod_plan_status ORs the status words of both workspaces (include/slod.h): directly after execute A alone,
    which ran in the healthy workspace 1, it still reports the failed execute of workspace 0; execute B, the next
    one in workspace 0, clears it."""
    _setenv(monkeypatch, "tw", {}, debug=False)
    fresh = _fresh(so, "scalar", "tw", {})
    ref, g, fields, hit = _case(so, "scalar", "negative")
    ids = _order(g)
    plan = g.plan(ids)
    plan.set_overlap(2)
    _run(plan)
    assert _status_of(plan)[0] == ERR_NUMERIC
    _upload(g, ref.base)
    ba, qa = _run(plan)
    assert _status_of(plan)[0] == ERR_NUMERIC
    bb, qb = _run(plan)
    plan.join()
    _assert_recovered(so, ref, plan, ids, bb, qb, fresh, "overlap B")
    plan.close()
    g.close()


# ---------------------------------------------------------------- 7: the exchange path resets the status on its own
@gpu
@pytest.mark.parametrize("n_pieces", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_execute_allgather_recovers(so, kind, n_pieces, monkeypatch):
    import slod_amd
    _setenv(monkeypatch, "tw", {}, debug=False)
    torch, dev = _torch()
    fresh = _fresh(so, "scalar", "tw", {}, reverse=False)
    ref, g, fields, hit = _case(so, "scalar", kind)
    ids = _order(g, reverse=False)
    plan = g.plan(ids)
    comm = slod_amd.Comm(slod_amd.Comm.unique_id(), 1, 0, 0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def run():
        b = torch.full((len(ids) * plan.stride,), float("nan"), dtype=torch.float64, device=dev)
        q = torch.full_like(b, float("nan"))
        torch.cuda.synchronize()
        plan.execute_allgather(comm, b.data_ptr(), q.data_ptr(), len(ids), n_pieces, s1.cuda_stream, s2.cuda_stream)
        torch.cuda.synchronize()
        return b, q

    run()
    code, msg = _status_of(plan)
    assert code == ERR_NUMERIC and "patch solve" in msg
    _upload(g, ref.base)
    b, q = run()
    assert _status_of(plan) == (0, "")
    n = len(fresh[0])                          # the plan's output size: the last patch's vectors end the slab
    assert np.array_equal(_bits(b)[:n], fresh[0]) and np.array_equal(_bits(q)[:n], fresh[1])
    assert torch.isnan(b[n:]).all() and torch.isnan(q[n:]).all()
    comm.close()
    plan.close()
    g.close()
