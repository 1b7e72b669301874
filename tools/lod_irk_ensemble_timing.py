#!/usr/bin/env python3
"""Time the two-stage implicit Runge-Kutta steppers on a coefficient ensemble next to what they replace, on BASELINE
configuration C2 (2-D Poisson, H = 1/32, n_sub 8, oversampling 2: 1024 unknowns per member, half bandwidth 165), K members
with D1e4 coefficients of their own (seeds SEED + k), for every K of --members, Gauss and Radau, heat and wave
(undamped, constant load, from u = 0 / from rest), per call of STEPS steps:

  ensemble           slod_lod_irk_heat_steps_ensemble_direct / slod_lod_irk_wave_steps_ensemble_direct on one complex factor
                     object of K members; the wave without and with the energies of every level
  sequential         K sequential slod_lod_irk_heat_steps_direct / slod_lod_irk_wave_steps_direct (n_rhs = 1) on the
                     de-interleaved members and their one-member factors; the wave without and with energies
  newmark_ensemble   the trapezoidal rule, slod_lod_newmark_steps_ensemble_direct (beta = 1/4, gamma = 1/2) without
                     energies, on the real factors of M + dt^2 / 4 A
dt = 0.7 / omega_1 of member 0 (slod_lod_eigs), as tools/lod_ensemble_wave_timing.py; for heat dt = 0.7 / lambda_1.

Launches of a step: 3 (right-hand side, complex sweeps, update), 5 with the energies, for any K; the sequential path
queues K times as many and waits K times per call.
Bytes a step must move per member (matrix words of 8 bytes on the shared pattern, both planes of the band of the complex
factor): A once for the right-hand side (the wave reads each word of A once for A u and A v); the factor twice (forward
and backward sweep); A and M once more for the energies; M again when damp_mass != 0 (not timed here).  The vectors are
1024 doubles and are left out.

HIP-event time of each call (median of --reps after a warm-up of every variant, the variants taken in turn inside every
repetition, with the least and the largest next to it; the events sit on the null stream and the calls end synchronised,
so they enclose the allocation of the workspace, the reset of the state and the one wait).  One JSON line per
(K, scheme); nothing is asserted.

  python tools/lod_irk_ensemble_timing.py [--reps 7] [--members 1 8 64]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-slod_amd"))

SEED = 20250614
C2 = dict(nref=5, n_sub=8, oversampling=2, spacedim=1, stabilize=1)
STEPS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 64])
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_irk_ensemble_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
    dev = torch.device("cuda", 0)
    kmax = max(args.members)
    g = slod_amd.Slod(n_problems=kmax, **C2)
    for k in range(kmax):
        t = torch.from_numpy(fill_coefficient(SEED + k, "D1e4", g.NE)).to(dev)
        g.set_coefficient_device(0, t.data_ptr(), t.numel(), problem=k)
        torch.cuda.synchronize()
    NP, cap = g.num_patches, g.lod_row_capacity()
    plan = g.plan(np.arange(kmax * NP, dtype=np.uint32))
    stride = plan.stride
    b = torch.zeros(kmax * NP * stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    plan.status()
    torch.cuda.synchronize()
    nfine, nval = (g.NE + 1) ** 2, NP * cap
    load = torch.zeros(nfine, dtype=torch.float64, device=dev)
    g.fem_rhs(None, load.data_ptr())
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        torch.cuda.synchronize()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def medians(fns):
        """per variant (median event ms, least, largest) of --reps runs, the variants in turn inside a repetition"""
        for fn in fns.values():
            fn()
        runs = {name: [] for name in fns}
        for _ in range(args.reps):
            for name, fn in fns.items():
                runs[name].append(timed(fn))
        return {name: (sorted(r)[len(r) // 2], min(r), max(r)) for name, r in runs.items()}

    lam1 = None
    for K in args.members:
        raw, A, M, S = (torch.zeros(nval, K, dtype=torch.float64, device=dev) for _ in range(4))
        cols = torch.zeros(nval, dtype=torch.int32, device=dev)
        mcols = torch.zeros_like(cols)
        R = torch.zeros(NP, K, dtype=torch.float64, device=dev)
        g.lod_matrix_ensemble(b.data_ptr(), q.data_ptr(), stride, K, raw.data_ptr(), cols.data_ptr())
        g.lod_mass_matrix_ensemble(b.data_ptr(), stride, K, M.data_ptr(), mcols.data_ptr())
        g.lod_matrix_symmetrize_ensemble(raw.data_ptr(), cols.data_ptr(), K, A.data_ptr())
        g.lod_rhs_ensemble(b.data_ptr(), stride, K, load.data_ptr(), R.data_ptr())
        torch.cuda.synchronize()
        if lam1 is None:                                                      # member 0 is the same for every K
            X = torch.zeros(NP, 5, dtype=torch.float64, device=dev)
            lam, _, _ = g.lod_eigs(A[:, 0].contiguous().data_ptr(), M[:, 0].contiguous().data_ptr(), cols.data_ptr(), 1,
                                   X.data_ptr(), n_block=5)
            lam1 = float(lam[0])
        dts = {1: 0.7 / lam1, 2: 0.7 / math.sqrt(lam1)}
        Ak, Mk, Rk = ([x[:, k].contiguous() for k in range(K)] for x in (A, M, R))
        # the trapezoidal rule on the ensemble: the second-order step the user has today
        dtw = dts[2]
        g.lod_matrix_combine_ensemble(1.0, M.data_ptr(), 0.25 * dtw * dtw, A.data_ptr(), K, S.data_ptr())
        torch.cuda.synchronize()
        fM = g.lod_factor_ensemble(M.data_ptr(), cols.data_ptr(), K)
        fS = g.lod_factor_ensemble(S.data_ptr(), cols.data_ptr(), K)
        U, V, Acc, A0 = (torch.zeros_like(R) for _ in range(4))
        g.lod_newmark_accel_ensemble_direct(fM, A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, U.data_ptr(), V.data_ptr(),
                                            A0.data_ptr(), d_load=R.data_ptr())
        u1, v1 = (torch.zeros(NP, dtype=torch.float64, device=dev) for _ in range(2))

        def newmark():
            U.zero_(), V.zero_(), Acc.copy_(A0)
            g.lod_newmark_steps_ensemble_direct(fS, A.data_ptr(), M.data_ptr(), cols.data_ptr(), dtw, STEPS, K, U.data_ptr(),
                                                V.data_ptr(), Acc.data_ptr(), d_load=R.data_ptr(), energies=False)

        for label in ("gauss", "radau"):
            fe, fs = {}, {}
            for order in (1, 2):
                alpha, beta = g.lod_irk_coefficients(label, order, dts[order])
                fe[order] = g.lod_factor_zldl_ensemble(A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, [alpha], [beta])
                fs[order] = [g.lod_factor_zldl(Ak[k].data_ptr(), Mk[k].data_ptr(), cols.data_ptr(), [alpha], [beta])
                             for k in range(K)]
            out = {}

            def heat_ens():
                U.zero_()
                g.lod_irk_heat_steps_ensemble(fe[1], label, A.data_ptr(), cols.data_ptr(), dts[1], STEPS, K, U.data_ptr(),
                                              d_load=R.data_ptr())

            def heat_seq():
                for k in range(K):
                    u1.zero_()
                    g.lod_irk_heat_steps(fs[1][k], label, Ak[k].data_ptr(), cols.data_ptr(), dts[1], STEPS, u1.data_ptr(),
                                         d_load=Rk[k].data_ptr())

            def wave_ens(energies):
                def run():
                    U.zero_(), V.zero_()
                    out["ens"] = g.lod_irk_wave_steps_ensemble(fe[2], label, A.data_ptr(), M.data_ptr(), cols.data_ptr(), dts[2],
                                                               STEPS, K, U.data_ptr(), V.data_ptr(), d_load=R.data_ptr(),
                                                               energies=energies)
                return run

            def wave_seq(energies):
                def run():
                    for k in range(K):
                        u1.zero_(), v1.zero_()
                        out["seq"] = g.lod_irk_wave_steps(fs[2][k], label, Ak[k].data_ptr(), Mk[k].data_ptr(), cols.data_ptr(),
                                                          dts[2], STEPS, u1.data_ptr(), v1.data_ptr(), d_load=Rk[k].data_ptr(),
                                                          energies=energies)
                return run

            t = medians({"heat_ensemble": heat_ens, "heat_sequential": heat_seq, "wave_ensemble": wave_ens(False),
                         "wave_sequential": wave_seq(False), "wave_ensemble_energy": wave_ens(True),
                         "wave_sequential_energy": wave_seq(True), "newmark_ensemble": newmark})
            # the last member's energies of the two paths are the same words
            same = bool(out["ens"][0][:, K - 1].tobytes() == out["seq"][0][:, 0].tobytes()
                        and out["ens"][1][:, K - 1].tobytes() == out["seq"][1][:, 0].tobytes())
            matrix_bytes, factor_bytes = 8 * nval, fe[2].info.bytes // K
            step_bytes = matrix_bytes + 2 * factor_bytes
            energy_bytes = step_bytes + 2 * matrix_bytes
            print(json.dumps({
                "n_members": K, "scheme": label, "steps_per_call": STEPS, "dt_heat": dts[1], "dt_wave": dts[2],
                "n": fe[2].info.n, "half_bandwidth": fe[2].info.half_bandwidth,
                "launches_per_step": {"ensemble": 3, "ensemble_energy": 5, "sequential": 3 * K, "sequential_energy": 5 * K},
                "matrix_bytes_per_member": matrix_bytes, "complex_factor_bytes_per_member": factor_bytes,
                "real_factor_bytes_per_member": fS.info.bytes // K,
                "step_bytes_per_member": step_bytes, "step_with_energies_bytes_per_member": energy_bytes,
                "call_event_ms_median_min_max": {name: list(v) for name, v in t.items()},
                "sequential_over_ensemble": {
                    "heat": t["heat_sequential"][0] / t["heat_ensemble"][0],
                    "wave": t["wave_sequential"][0] / t["wave_ensemble"][0],
                    "wave_energy": t["wave_sequential_energy"][0] / t["wave_ensemble_energy"][0]},
                "irk_wave_step_over_newmark_step": t["wave_ensemble"][0] / t["newmark_ensemble"][0],
                "wave_step_gbytes_per_s": K * step_bytes / (t["wave_ensemble"][0] / STEPS) * 1e-6,
                "wave_step_with_energies_gbytes_per_s": K * energy_bytes / (t["wave_ensemble_energy"][0] / STEPS) * 1e-6,
                "last_member_energies_equal_single_call": same}), flush=True)
            for x in [fe[1], fe[2]] + fs[1] + fs[2]:
                x.close()
        for x in (fM, fS):
            x.close()


if __name__ == "__main__":
    main()
