#!/usr/bin/env python3
"""Time the sponge layer, a third damping matrix D in the wave steppers and the frequency response, on BASELINE
configuration C2 (2-D Poisson, H = 1/32, n_sub 8, oversampling 2: 1024 patches = 1024 rows, D1e4 coefficient), with the
sponge of width 0.25 and sigma_max = 4 sqrt(lam_1).

  undamped  ms per step of slod_lod_newmark_steps_direct (trapezoidal) and slod_lod_irk_wave_steps_direct (Gauss), n_rhs 1
            and 16, and ms per frequency of slod_lod_harmonic_response (64 frequencies), all without D: the calls and the
            kernel instantiations of the parent commit.  With --undamped-only the tool stops here; with --tree DIR it imports
            the package (and loads the library) of another checkout, so that the parent commit and this tree are timed by the
            same code, alternating.
  damped    the same steps with D against the steps without, n_rhs 1 and 16, with and without the energies; next to the
            difference the spread (max - min) of the undamped run, the noise floor of the measurement.
  factor    slod_lod_factor_create_zldl3 against slod_lod_factor_create_zldl, 1 and 64 members.
  sweep     slod_lod_harmonic_response with D (six products, five quantities) against the sweep without.
  bytes     what the extra row product must move per step and column: the words of D and the column indices are shared with
            the M chain, so with damp_mass = 0 the damped step reads D in place of nothing, else D on top of M.
Wall-clock times around a device synchronisation: minimum, median and maximum of --reps runs after a warm-up.  No time and
no ratio is asserted anywhere.  One JSON line per measurement, printed and, with --out, appended to that file.

  python tools/lod_sponge_timing.py [--reps 9] [--steps 8] [--out profiles/lod_sponge_timing.txt]
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
    ap.add_argument("--undamped-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.tree, "dealii-slod_amd"))
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_sponge_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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

    def stats(fn, per=1):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
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
    w1 = float(np.sqrt(low[0]))
    dt, K = 0.5 / w1, args.steps
    emit({"rows": nrow, "dt": dt, "steps_per_call": K, "reps": args.reps, "row_capacity": cap})

    g.lod_matrix_combine(1.0, M, 0.25 * dt * dt, A, S.data_ptr())
    torch.cuda.synchronize()
    f_nm = g.lod_factor(S.data_ptr(), Cc)
    aw, bw = g.lod_irk_coefficients("gauss", 2, dt)
    f_irk = g.lod_factor_zldl(A, M, Cc, [aw], [bw])
    omegas = np.linspace(0.5 * w1, 8.0 * w1, 64)
    load = torch.from_numpy(np.random.default_rng(5).uniform(-1.0, 1.0, (nrow, 1))).to(dev)
    ur, ui = torch.zeros(nrow, 64, dtype=torch.float64, device=dev), torch.zeros(nrow, 64, dtype=torch.float64, device=dev)

    def loops(n, energies, f_n, f_i, **damp):
        rng = np.random.default_rng(7)
        U = torch.from_numpy(rng.uniform(-1.0, 1.0, (nrow, n))).to(dev)
        V, Acc = torch.zeros_like(U), torch.zeros_like(U)
        return {
            "newmark": lambda: g.lod_newmark_steps_direct(f_n, A, M, Cc, dt, K, U.data_ptr(), V.data_ptr(), Acc.data_ptr(), n_rhs=n,
                                                          energies=energies, **damp),
            "irk_wave": lambda: g.lod_irk_wave_steps(f_i, "gauss", A, M, Cc, dt, K, U.data_ptr(), V.data_ptr(), n_rhs=n,
                                                     energies=energies, **damp)}

    def sweep(**damp):
        return lambda: g.lod_harmonic_response(A, M, Cc, omegas, load.data_ptr(), None, ur.data_ptr(), ui.data_ptr(),
                                               damp_mass=0.02 * w1, **damp)

    for n in (1, 16):
        for name, fn in loops(n, False, f_nm, f_irk).items():
            emit({"undamped": name, "n_rhs": n, "ms_per_step": stats(fn, K)})
    emit({"undamped": "harmonic_response", "n_freq": 64, "ms_per_frequency": stats(sweep(), 64)})
    if args.undamped_only:
        return

    # the sponge and the factors of the damped step matrices
    sigma = torch.from_numpy(slod_amd.sponge_profile(g.NE, 0.25, 4.0 * w1)).to(dev)
    dmat = torch.zeros_like(raw)
    g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, dmat.data_ptr(), mcols.data_ptr(), d_rho=sigma.data_ptr())
    g.lod_matrix_combine(1.0, S.data_ptr(), 0.5 * dt, dmat.data_ptr(), S.data_ptr())
    torch.cuda.synchronize()
    Dp = dmat.data_ptr()
    f_nm3 = g.lod_factor(S.data_ptr(), Cc)
    zw = g.lod_irk_damping_coefficient("gauss", dt)
    f_irk3 = g.lod_factor_zldl3(A, M, Dp, Cc, [aw], [bw], [zw])
    for n in (1, 16):
        for energies in (False, True):
            plain, damped = loops(n, energies, f_nm, f_irk), loops(n, energies, f_nm3, f_irk3, d_damping=Dp)
            for name in plain:
                t0, t1 = stats(plain[name], K), stats(damped[name], K)
                emit({"damped": name, "n_rhs": n, "energies": energies, "damped_ms_per_step": t1, "undamped_ms_per_step": t0,
                      "extra_us_per_step_median": (t1["median"] - t0["median"]) * 1e3, "undamped_spread_us": (t0["max"] - t0["min"]) * 1e3})

    for members in (1, 64):
        al, be = [1.0 + 1j * (w * 1e-3 / w1) for w in omegas[:members]], [-(w * w) + 1j * (w * 0.02 * w1) for w in omegas[:members]]
        ga = [1j * w for w in omegas[:members]]

        def two():
            g.lod_factor_zldl(A, M, Cc, al, be).close()

        def three():
            g.lod_factor_zldl3(A, M, Dp, Cc, al, be, ga).close()
        t2, t3 = stats(two), stats(three)
        emit({"factor": "zldl3 against zldl", "members": members, "zldl3_ms": t3, "zldl_ms": t2,
              "extra_us_median": (t3["median"] - t2["median"]) * 1e3, "zldl_spread_us": (t2["max"] - t2["min"]) * 1e3})

    t0, t1 = stats(sweep(), 64), stats(sweep(d_damping=Dp), 64)
    emit({"sweep": "harmonic_response, 64 frequencies", "damped_ms_per_frequency": t1, "undamped_ms_per_frequency": t0,
          "extra_us_per_frequency_median": (t1["median"] - t0["median"]) * 1e3, "undamped_spread_us": (t0["max"] - t0["min"]) * 1e3})

    used = int((cols.cpu().numpy().view(np.uint32) < NP).sum())
    emit({"bytes": "the D chain of one right-hand side, per column", "matrix_words_bytes": used * 8, "column_index_bytes_shared": used * 4,
          "vector_bytes_shared_with_the_M_or_A_chain": nrow * 8, "used_slots": used, "slots": NP * cap})
    for f in (f_nm, f_irk, f_nm3, f_irk3):
        f.close()


if __name__ == "__main__":
    main()
