#!/usr/bin/env python3
"""Time the Newmark stepper on an ensemble factor next to what it replaces, on BASELINE configuration C2 (2-D Poisson,
H = 1/32, n_sub 8, oversampling 2: 1024 unknowns per member, half bandwidth 165), K members with D1e4 coefficients of
their own (seeds SEED + k), all in one run and for every K of --members.  A trapezoidal step (beta = 1/4, gamma = 1/2,
undamped, constant load, from rest) of all members, per step of a call of STEPS steps:

  ensemble          slod_lod_newmark_steps_ensemble_direct without energies
  ensemble+energy   the same with kinetic and potential energy of every level
  sequential        K sequential slod_lod_newmark_steps_direct on the de-interleaved members and their single factors,
                    without and with energies
  theta             a Crank-Nicolson step of slod_lod_theta_steps_ensemble_direct on the factor of M + dt/2 A
dt = 0.7 / omega_1 of member 0 (slod_lod_eigs), as tools/lod_ensemble_direct_timing.py.

Bytes a step must move per member (matrix words of 8 bytes on the shared pattern, the band of the factor):
  A once for the right-hand side; A and M once more for the energies; M again when damp_mass != 0 (not timed here); the
  factor twice (forward and backward sweep).  The vectors are 1024 doubles and are left out.

HIP-event time of each call (median of --reps after a warm-up of every variant, the variants taken in turn inside every
repetition, with the least and the largest in event_ms_range; the events sit on the null stream and the calls end
synchronised, so they enclose the allocation of the workspace, the reset of the state and the one wait).  One JSON line
per K; nothing is asserted.

  python tools/lod_ensemble_wave_timing.py [--reps 7] [--members 1 8 64]
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
STEPS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 64])
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_ensemble_wave_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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
        """per variant (median event ms, [least, largest]) of --reps runs, the variants in turn inside a repetition"""
        for fn in fns.values():
            fn()
        runs = {name: [] for name in fns}
        for _ in range(args.reps):
            for name, fn in fns.items():
                runs[name].append(timed(fn))
        return {name: (sorted(r)[len(r) // 2], [min(r), max(r)]) for name, r in runs.items()}

    dt = None
    for K in args.members:
        raw, A, M, S, T = (torch.zeros(nval, K, dtype=torch.float64, device=dev) for _ in range(5))
        cols = torch.zeros(nval, dtype=torch.int32, device=dev)
        mcols = torch.zeros_like(cols)
        R = torch.zeros(NP, K, dtype=torch.float64, device=dev)
        g.lod_matrix_ensemble(b.data_ptr(), q.data_ptr(), stride, K, raw.data_ptr(), cols.data_ptr())
        g.lod_mass_matrix_ensemble(b.data_ptr(), stride, K, M.data_ptr(), mcols.data_ptr())
        g.lod_matrix_symmetrize_ensemble(raw.data_ptr(), cols.data_ptr(), K, A.data_ptr())
        g.lod_rhs_ensemble(b.data_ptr(), stride, K, load.data_ptr(), R.data_ptr())
        torch.cuda.synchronize()
        if dt is None:                                                        # member 0 is the same for every K
            X = torch.zeros(NP, 5, dtype=torch.float64, device=dev)
            lam, _, _ = g.lod_eigs(A[:, 0].contiguous().data_ptr(), M[:, 0].contiguous().data_ptr(), cols.data_ptr(), 1,
                                   X.data_ptr(), n_block=5)
            dt = 0.7 / math.sqrt(lam[0])
        g.lod_matrix_combine_ensemble(1.0, M.data_ptr(), 0.25 * dt * dt, A.data_ptr(), K, S.data_ptr())
        g.lod_matrix_combine_ensemble(1.0, M.data_ptr(), 0.5 * dt, A.data_ptr(), K, T.data_ptr())
        torch.cuda.synchronize()
        fM = g.lod_factor_ensemble(M.data_ptr(), cols.data_ptr(), K)
        fS = g.lod_factor_ensemble(S.data_ptr(), cols.data_ptr(), K)
        fT = g.lod_factor_ensemble(T.data_ptr(), cols.data_ptr(), K)
        Ak, Mk, Sk, Rk = ([x[:, k].contiguous() for k in range(K)] for x in (A, M, S, R))
        singles = [g.lod_factor(Sk[k].data_ptr(), cols.data_ptr()) for k in range(K)]
        U, V, Acc, A0 = (torch.zeros_like(R) for _ in range(4))
        g.lod_newmark_accel_ensemble_direct(fM, A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, U.data_ptr(), V.data_ptr(),
                                            A0.data_ptr(), d_load=R.data_ptr())
        a0 = [A0[:, k].contiguous() for k in range(K)]
        u1, v1, a1 = (torch.zeros(NP, dtype=torch.float64, device=dev) for _ in range(3))
        out = {}

        def ens(energies):
            def run():
                U.zero_(), V.zero_(), Acc.copy_(A0)
                out["ens"] = g.lod_newmark_steps_ensemble_direct(fS, A.data_ptr(), M.data_ptr(), cols.data_ptr(), dt, STEPS, K,
                                                                 U.data_ptr(), V.data_ptr(), Acc.data_ptr(), d_load=R.data_ptr(),
                                                                 energies=energies)
            return run

        def seq(energies):
            def run():
                for k in range(K):
                    u1.zero_(), v1.zero_(), a1.copy_(a0[k])
                    out["seq"] = g.lod_newmark_steps_direct(singles[k], Ak[k].data_ptr(), Mk[k].data_ptr(), cols.data_ptr(), dt, STEPS,
                                                            u1.data_ptr(), v1.data_ptr(), a1.data_ptr(), d_load=Rk[k].data_ptr(),
                                                            energies=energies)
            return run

        def theta():
            U.zero_()
            g.lod_theta_steps_ensemble_direct(fT, A.data_ptr(), cols.data_ptr(), dt, 0.5, STEPS, K, U.data_ptr(), d_load=R.data_ptr())

        t = medians({"ensemble": ens(False), "ensemble_energy": ens(True), "sequential": seq(False),
                     "sequential_energy": seq(True), "theta_ensemble": theta})
        # the last member's energies of the two paths are the same words
        same = bool(out["ens"][0][:, K - 1].tobytes() == out["seq"][0][:, 0].tobytes()
                    and out["ens"][1][:, K - 1].tobytes() == out["seq"][1][:, 0].tobytes())
        matrix_bytes, factor_bytes = 8 * nval, fS.info.bytes // K
        step_bytes = matrix_bytes + 2 * factor_bytes
        energy_bytes = step_bytes + 2 * matrix_bytes
        ms = {name: v[0] / STEPS for name, v in t.items()}
        print(json.dumps({
            "n_members": K, "dt": dt, "steps_per_call": STEPS, "n": fS.info.n, "half_bandwidth": fS.info.half_bandwidth,
            "matrix_bytes_per_member": matrix_bytes, "factor_bytes_per_member": factor_bytes,
            "step_bytes_per_member": step_bytes, "step_with_energies_bytes_per_member": energy_bytes,
            "mass_damping_adds_bytes_per_member": matrix_bytes,
            "step_ensemble_event_ms": ms["ensemble"], "step_ensemble_energy_event_ms": ms["ensemble_energy"],
            "step_sequential_event_ms": ms["sequential"], "step_sequential_energy_event_ms": ms["sequential_energy"],
            "cn_step_theta_ensemble_event_ms": ms["theta_ensemble"],
            "speedup_over_sequential": ms["sequential"] / ms["ensemble"],
            "speedup_over_sequential_with_energies": ms["sequential_energy"] / ms["ensemble_energy"],
            "newmark_over_theta_step": ms["ensemble"] / ms["theta_ensemble"],
            "step_gbytes_per_s": K * step_bytes / ms["ensemble"] * 1e-6,
            "step_with_energies_gbytes_per_s": K * energy_bytes / ms["ensemble_energy"] * 1e-6,
            "last_member_energies_equal_single_call": same,
            "call_event_ms_range": {name: v[1] for name, v in t.items()}}), flush=True)
        for x in [fM, fS, fT] + singles:
            x.close()


if __name__ == "__main__":
    main()
