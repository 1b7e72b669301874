#!/usr/bin/env python3
"""Time the record of the time loops on the LOD space (slod_lod_time_record_arm) on BASELINE configuration C2 (2-D Poisson,
H = 1/32, n_sub 8, oversampling 2: 1024 patches = 1024 rows, D1e4 coefficient).

  unarmed   ms per step of slod_lod_newmark_steps_direct (trapezoidal), slod_lod_theta_steps_direct (theta = 1/2) and
            slod_lod_irk_wave_steps_direct (Gauss), no record armed, n_rhs 1 and 16: one call of --steps steps divided by
            --steps.  With --unarmed-only the tool stops here; with --tree DIR it imports the package (and loads the
            library) of another checkout, so that the parent commit and this tree are timed by the same code, alternating.
  armed     the same steps with a record of 1, 16 and 256 nodal receivers (every = 1, u; the wave loops u and v), the
            Newmark ensemble step at K = 64 (the members are copies of the one matrix pair) with 16 receivers, and the
            added time per recorded step.
  replaced  what the record replaces: the same 64-step trapezoidal run as 64 calls of n_steps = 1, each followed by
            slod_lod_reconstruct_multi and a copy of the receiver nodes to the host; against one armed call and one copy.
Wall-clock times around a device synchronisation: minimum, median and maximum of --reps runs after a warm-up.  No time and
no ratio is asserted anywhere.  One JSON line per measurement, printed and, with --out, appended to that file.

  python tools/lod_receivers_timing.py [--reps 9] [--steps 8] [--out profiles/lod_receivers_timing.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

SEED = 20250614
C2 = dict(nref=5, n_sub=8, oversampling=2, spacedim=1, stabilize=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--unarmed-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.tree, "dealii-slod_amd"))
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_receivers_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
    dev = torch.device("cuda", 0)
    g = slod_amd.Slod(**C2)
    t = torch.from_numpy(fill_coefficient(SEED, "D1e4", g.NE)).to(dev)
    g.set_coefficient_device(0, t.data_ptr(), t.numel())
    ids = np.arange(g.num_patches, dtype=np.uint32)
    plan = g.plan(ids)
    b = torch.zeros(len(ids) * plan.stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    NP, cap = g.num_patches, g.lod_row_capacity()
    nrow = NP
    raw = torch.zeros(NP * cap, dtype=torch.float64, device=dev)
    sym, mass, S = torch.zeros_like(raw), torch.zeros_like(raw), torch.zeros_like(raw)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    mcols = torch.zeros_like(cols)
    g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, raw.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, mass.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize(raw.data_ptr(), cols.data_ptr(), sym.data_ptr())
    torch.cuda.synchronize()
    A, M, Cc = sym.data_ptr(), mass.data_ptr(), cols.data_ptr()

    def emit(record):
        record = dict(record, tree=args.label)
        line = json.dumps(record)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def stats(fn, per=1, arm=None):
        for _ in range(2):
            if arm:
                arm()
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            if arm:
                arm()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / per)
        ms.sort()
        return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}

    fc = g.lod_factor(A, Cc)
    X = torch.zeros(nrow, 16, dtype=torch.float64, device=dev)
    low = g.lod_eigs_direct(fc, A, M, Cc, 8, X.data_ptr(), n_block=16, ld_x=16)[0]
    fc.close()
    dt, K = 0.5 / float(np.sqrt(low[0])), args.steps
    emit({"rows": nrow, "dt": dt, "steps_per_call": K, "reps": args.reps})

    g.lod_matrix_combine(1.0, M, 0.25 * dt * dt, A, S.data_ptr())
    torch.cuda.synchronize()
    f_nm = g.lod_factor(S.data_ptr(), Cc)
    S2 = torch.zeros_like(S)
    g.lod_matrix_combine(1.0, M, 0.5 * dt, A, S2.data_ptr())
    torch.cuda.synchronize()
    f_th = g.lod_factor(S2.data_ptr(), Cc)
    aw, bw = g.lod_irk_coefficients("gauss", 2, dt)
    f_irk = g.lod_factor_zldl(A, M, Cc, [aw], [bw])

    def loops(n, steps=K):
        rng = np.random.default_rng(7)
        U = torch.from_numpy(rng.uniform(-1.0, 1.0, (nrow, n))).to(dev)
        V, Acc = torch.zeros_like(U), torch.zeros_like(U)
        return U, V, Acc, {
            "newmark": (lambda: g.lod_newmark_steps_direct(f_nm, A, M, Cc, dt, steps, U.data_ptr(), V.data_ptr(), Acc.data_ptr(), n_rhs=n,
                                                           energies=False), True),
            "theta": (lambda: g.lod_theta_steps_direct(f_th, A, Cc, dt, 0.5, steps, U.data_ptr(), n_rhs=n), False),
            "irk_wave": (lambda: g.lod_irk_wave_steps(f_irk, "gauss", A, M, Cc, dt, steps, U.data_ptr(), V.data_ptr(), n_rhs=n,
                                                      energies=False), True)}

    unarmed = {}
    for n in (1, 16):
        for name, (fn, _) in loops(n)[3].items():
            unarmed[name, n] = stats(fn, K)
            emit({"unarmed": name, "n_rhs": n, "ms_per_step": unarmed[name, n]})
    if args.unarmed_only:
        return

    NEp = g.NE + 1
    rng = np.random.default_rng(9)
    for n_recv in (1, 16, 256):
        nodes = rng.choice(NEp * NEp, n_recv, replace=False)
        recv = g.lod_receivers([[(int(nd), 0, 1.0)] for nd in nodes], b.data_ptr(), plan.stride)
        for n in (1, 16):
            trace = torch.zeros((K + 1) * 2 * n_recv * n, dtype=torch.float64, device=dev)
            for name, (fn, has_v) in loops(n)[3].items():
                what = slod_amd.RECORD_U | slod_amd.RECORD_V if has_v else slod_amd.RECORD_U
                arm = lambda: g.lod_time_record(recv, trace.data_ptr(), capacity=K + 1, what=what, columns=n)
                t_arm = stats(fn, K, arm)
                emit({"armed": name, "n_rhs": n, "receivers": n_recv, "nnz": int(recv.info.nnz), "ms_per_step": t_arm,
                      "added_us_per_recorded_step_median": (t_arm["median"] - unarmed[name, n]["median"]) * 1e3 * K / (K + 1),
                      "unarmed_spread_us": (unarmed[name, n]["max"] - unarmed[name, n]["min"]) * 1e3})
        recv.close()

    # the ensemble step at K = 64: the members are copies of the one matrix pair and of the one slab (member_stride 0)
    KE = 64
    Ae, Me = sym.repeat_interleave(KE).contiguous(), mass.repeat_interleave(KE).contiguous()
    Se = torch.zeros_like(Ae)
    g.lod_matrix_combine_ensemble(1.0, Me.data_ptr(), 0.25 * dt * dt, Ae.data_ptr(), KE, Se.data_ptr())
    torch.cuda.synchronize()
    fe = g.lod_factor_ensemble(Se.data_ptr(), Cc, KE)
    Ue = torch.from_numpy(rng.uniform(-1.0, 1.0, (nrow, KE))).to(dev)
    Ve, Ace = torch.zeros_like(Ue), torch.zeros_like(Ue)
    ens = lambda: g.lod_newmark_steps_ensemble_direct(fe, Ae.data_ptr(), Me.data_ptr(), Cc, dt, K, KE, Ue.data_ptr(), Ve.data_ptr(),
                                                      Ace.data_ptr(), energies=False)
    t_un = stats(ens, K)
    nodes = rng.choice(NEp * NEp, 16, replace=False)
    recv = g.lod_receivers([[(int(nd), 0, 1.0)] for nd in nodes], b.data_ptr(), plan.stride, n_members=KE, member_stride=0)
    trace = torch.zeros((K + 1) * 2 * 16 * KE, dtype=torch.float64, device=dev)
    arm = lambda: g.lod_time_record(recv, trace.data_ptr(), capacity=K + 1, what=3, columns=KE)
    t_arm = stats(ens, K, arm)
    emit({"ensemble": "newmark", "members": KE, "receivers": 16, "unarmed_ms_per_step": t_un, "armed_ms_per_step": t_arm,
          "added_us_per_recorded_step_median": (t_arm["median"] - t_un["median"]) * 1e3 * K / (K + 1)})
    recv.close()
    fe.close()

    # what the record replaces: 64 calls of one step, each with a full reconstruction and a copy of the receiver nodes
    steps, n, n_recv = 64, 1, 16
    nodes = np.sort(rng.choice(NEp * NEp, n_recv, replace=False))
    idx = torch.from_numpy(nodes).to(dev)
    recv = g.lod_receivers([[(int(nd), 0, 1.0)] for nd in nodes], b.data_ptr(), plan.stride)
    U0 = torch.from_numpy(rng.uniform(-1.0, 1.0, (nrow, n))).to(dev)
    U, V, Acc = U0.clone(), torch.zeros_like(U0), torch.zeros_like(U0)
    fine = torch.zeros(n, NEp * NEp, dtype=torch.float64, device=dev)
    trace = torch.zeros((steps + 1) * n_recv * n, dtype=torch.float64, device=dev)

    def reset():
        U.copy_(U0), V.zero_(), Acc.zero_()

    def cut():
        reset()
        out = np.zeros((steps + 1, n_recv))
        for k in range(steps + 1):
            if k:
                g.lod_newmark_steps_direct(f_nm, A, M, Cc, dt, 1, U.data_ptr(), V.data_ptr(), Acc.data_ptr(), n_rhs=n, energies=False)
            g.lod_reconstruct_multi(b.data_ptr(), plan.stride, U.data_ptr(), n, n, fine.data_ptr(), NEp * NEp)
            out[k] = fine[0, idx].cpu().numpy()
        return out

    def whole():
        reset()
        g.lod_time_record(recv, trace.data_ptr(), capacity=steps + 1, columns=n)
        g.lod_newmark_steps_direct(f_nm, A, M, Cc, dt, steps, U.data_ptr(), V.data_ptr(), Acc.data_ptr(), n_rhs=n, energies=False)
        return trace.cpu().numpy().reshape(steps + 1, n_recv)

    same = bool(np.array_equal(cut().view(np.uint64), whole().view(np.uint64)))
    t_cut, t_whole = stats(cut), stats(whole)
    emit({"replaced": "64 trapezoidal steps, 16 receivers, n_rhs 1", "traces_equal_as_words": same,
          "cut_into_single_steps_ms": t_cut, "one_armed_call_ms": t_whole, "ratio_median": t_cut["median"] / t_whole["median"]})


if __name__ == "__main__":
    main()
