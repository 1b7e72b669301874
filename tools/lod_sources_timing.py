#!/usr/bin/env python3
"""Time the source of the time loops on the LOD space (slod_lod_time_source_arm) on BASELINE configuration C2 (2-D Poisson,
H = 1/32, n_sub 8, oversampling 2: 1024 patches = 1024 rows, D1e4 coefficient).

  unarmed   ms per step of slod_lod_newmark_steps_direct (trapezoidal), slod_lod_theta_steps_direct (theta = 1/2) and
            slod_lod_irk_wave_steps_direct (Gauss), no source armed, n_rhs 1 and 16: one call of --steps steps divided by
            --steps.  With --unarmed-only the tool stops here; with --tree DIR it imports the package (and loads the
            library) of another checkout, so that the parent commit and this tree are timed by the same code, alternating.
  armed     the same steps driven by 1, 16 and 256 nodal sources, against the un-armed step that reads materialised loads
            of the same content (slod_lod_inject_multi, sample by sample): the difference is the cost of the inject launch;
            next to it the spread (max - min) of the materialised run, the noise floor of the measurement.
  memory    the device bytes of the loads of a 4096-step, 16-column run at C2, materialised and as a signal of 16 sources.
Wall-clock times around a device synchronisation: minimum, median and maximum of --reps runs after a warm-up.  No time and
no ratio is asserted anywhere.  One JSON line per measurement, printed and, with --out, appended to that file.

  python tools/lod_sources_timing.py [--reps 9] [--steps 8] [--out profiles/lod_sources_timing.txt]
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
        raise SystemExit("lod_sources_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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

    def loops(n, load=None):
        """The three steps on n columns; load: None or a device tensor [samples][nrow][n] the call reads as d_load."""
        rng = np.random.default_rng(7)
        U = torch.from_numpy(rng.uniform(-1.0, 1.0, (nrow, n))).to(dev)
        V, Acc = torch.zeros_like(U), torch.zeros_like(U)
        step = {} if load is None else dict(d_load=load.data_ptr(), ld_load=n, load_step_stride=nrow * n)
        stage = {} if load is None else dict(d_load=load.data_ptr(), ld_load=n, load_stage_stride=nrow * n)
        return {
            "newmark": lambda: g.lod_newmark_steps_direct(f_nm, A, M, Cc, dt, K, U.data_ptr(), V.data_ptr(), Acc.data_ptr(), n_rhs=n,
                                                          energies=False, **step),
            "theta": lambda: g.lod_theta_steps_direct(f_th, A, Cc, dt, 0.5, K, U.data_ptr(), n_rhs=n, **step),
            "irk_wave": lambda: g.lod_irk_wave_steps(f_irk, "gauss", A, M, Cc, dt, K, U.data_ptr(), V.data_ptr(), n_rhs=n,
                                                     energies=False, **stage)}

    for n in (1, 16):
        for name, fn in loops(n).items():
            emit({"unarmed": name, "n_rhs": n, "ms_per_step": stats(fn, K)})
    if args.unarmed_only:
        return

    NEp = g.NE + 1
    rng = np.random.default_rng(9)
    ns = 2 * K                                             # samples: enough for every loop (K + 1 or 2 K)
    for n_src in (1, 16, 256):
        nodes = rng.choice(NEp * NEp, n_src, replace=False)
        recv = g.lod_receivers([[(int(nd), 0, 1.0)] for nd in nodes], b.data_ptr(), plan.stride)
        src = g.lod_sources(recv)
        recv.close()
        for n in (1, 16):
            sig = torch.from_numpy(rng.uniform(-1.0, 1.0, (ns, n_src, n))).to(dev)
            mat = torch.zeros(ns, nrow, n, dtype=torch.float64, device=dev)
            for j in range(ns):
                src.inject(sig[j].data_ptr(), mat[j].data_ptr(), n_rhs=n)
            torch.cuda.synchronize()
            arm = lambda: g.lod_time_source(src, sig.data_ptr(), n_samples=ns, columns=n)
            plain, read = loops(n), loops(n, mat)
            for name in plain:
                t_mat, t_arm = stats(read[name], K), stats(plain[name], K, arm)
                emit({"armed": name, "n_rhs": n, "sources": n_src, "nnz": int(src.info.nnz), "rows_touched": int(src.info.n_rows_touched),
                      "armed_ms_per_step": t_arm, "materialised_ms_per_step": t_mat,
                      "inject_us_per_step_median": (t_arm["median"] - t_mat["median"]) * 1e3,
                      "materialised_spread_us": (t_mat["max"] - t_mat["min"]) * 1e3})
        src.close()

    steps, ncol, n_src = 4096, 16, 16
    emit({"memory": "C2, 4096 steps, 16 columns, 16 sources", "materialised_theta_newmark_bytes": (steps + 1) * nrow * ncol * 8,
          "materialised_irk_bytes": 2 * steps * nrow * ncol * 8, "signal_theta_newmark_bytes": (steps + 1) * n_src * ncol * 8,
          "signal_irk_bytes": 2 * steps * n_src * ncol * 8, "armed_workspace_bytes": 2 * nrow * ncol * 8})


if __name__ == "__main__":
    main()
