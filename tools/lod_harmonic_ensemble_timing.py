#!/usr/bin/env python3
"""Time the frequency response of a coefficient ensemble on BASELINE configuration C2 (2-D Poisson, H = 1/32, n_sub 8,
oversampling 2: 1024 patches = 1024 rows, half bandwidth 165, D1e4 coefficient) for F = 16 frequencies and K = 1, 8, 64
members, one load column per member.  Member k is (1 + k / 64) times the pair (sym(A_LOD), M_LOD): the matrices differ,
the spectrum and the growth do not.  The frequencies are evenly spaced in [sqrt(lambda_1) / 2, 2 sqrt(lambda_8)] (lambda
from slod_lod_eigs_direct), the damping is dm = 0.02 sqrt(lambda_1), ds = 1e-3 / sqrt(lambda_1).

  ensemble    slod_lod_harmonic_response_ensemble, the whole call: ceil(K F / 64) chunks of at most 64 factor members
  sequential  K calls of slod_lod_harmonic_response on the de-interleaved matrices of the members, F frequencies each:
              the yardstick, what the library offered before
  factor      slod_lod_factor_create_zldl_ensemble on the first chunk of the call (and its destroy)
  solve       slod_lod_factor_solve_complex_ensemble on that factor, rhs_members = K
  residual    (ensemble - chunks (factor + solve)) / chunks: the four products in one launch, the residual and quantity
              kernels and the read-back, per chunk
Launches are counted from the code, per chunk of nb = rows / 16 block columns: the factor nb + 7, the solve 1, the
residual step 3 in the ensemble call and 6 in the single call.  residual_matrix_bytes is what k_harmonic_apply must
stream per chunk: every (row, column) item reads its own cap words of the member's matrix in each of the four products.
Wall-clock times around a device synchronisation: minimum, median and maximum of --reps runs after a warm-up.  No time
and no ratio is asserted anywhere.  One JSON line per measurement, printed and, with --out, appended to that file.

  python tools/lod_harmonic_ensemble_timing.py [--reps 5] [--out profiles/lod_harmonic_ensemble_timing.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-slod_amd"))

SEED = 20250614
C2 = dict(nref=5, n_sub=8, oversampling=2, spacedim=1, stabilize=1)
F, CHUNK = 16, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_harmonic_ensemble_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
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
    nrow, nval = NP, NP * cap
    raw = torch.zeros(nval, dtype=torch.float64, device=dev)
    sym, mass = torch.zeros_like(raw), torch.zeros_like(raw)
    cols = torch.zeros(nval, dtype=torch.int32, device=dev)
    mcols = torch.zeros_like(cols)
    g.lod_matrix(ids, b.data_ptr(), q.data_ptr(), plan.stride, raw.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix(ids, b.data_ptr(), plan.stride, mass.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize(raw.data_ptr(), cols.data_ptr(), sym.data_ptr())
    torch.cuda.synchronize()

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def stats(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}

    fc = g.lod_factor(sym.data_ptr(), cols.data_ptr())
    X = torch.zeros(nrow, 16, dtype=torch.float64, device=dev)
    low = g.lod_eigs_direct(fc, sym.data_ptr(), mass.data_ptr(), cols.data_ptr(), 8, X.data_ptr(), n_block=16, ld_x=16)[0]
    fc.close()
    w_lo, w_hi = 0.5 * float(np.sqrt(low[0])), 2.0 * float(np.sqrt(low[7]))
    dm, ds = 0.02 * float(np.sqrt(low[0])), 1e-3 / float(np.sqrt(low[0]))
    omegas = np.linspace(w_lo, w_hi, F)
    alpha, beta = 1.0 + 1j * (omegas * ds), -(omegas * omegas) + 1j * (omegas * dm)
    nb = (nrow + 15) // 16
    emit({"rows": nrow, "row_capacity": cap, "block_columns": nb, "n_freq": F, "omega_range": [w_lo, w_hi], "damp_mass": dm,
          "damp_stiff": ds, "reps": args.reps})

    for K in (1, 8, 64):
        scale = torch.tensor([1.0 + k / 64.0 for k in range(K)], dtype=torch.float64, device=dev)
        A, M = (sym[:, None] * scale[None, :]).contiguous(), (mass[:, None] * scale[None, :]).contiguous()
        singles = [(A[:, k].contiguous(), M[:, k].contiguous()) for k in range(K)]
        B = torch.from_numpy(np.random.default_rng(7).uniform(-1.0, 1.0, (nrow, K))).to(dev)
        ur, ui = (torch.zeros(nrow, F * K, dtype=torch.float64, device=dev) for _ in range(2))
        sr, si = (torch.zeros(nrow, F, dtype=torch.float64, device=dev) for _ in range(2))
        out = {}

        def ensemble():
            out["res"], out["growth"], out["q"] = g.lod_harmonic_response_ensemble(
                A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, omegas, B.data_ptr(), None, ur.data_ptr(), ui.data_ptr(),
                damp_mass=dm, damp_stiff=ds)

        def sequential():
            for k in range(K):
                g.lod_harmonic_response(singles[k][0].data_ptr(), singles[k][1].data_ptr(), cols.data_ptr(), omegas, B.data_ptr() + 8 * k,
                                        None, sr.data_ptr(), si.data_ptr(), damp_mass=dm, damp_stiff=ds, ld_load=K)

        # the first chunk of the call: min(64, F K) flat members = whole frequencies when K divides 64
        members = min(CHUNK, F * K)
        n_coef = members // K
        chunks = (F * K + CHUNK - 1) // CHUNK

        def factor():
            g.lod_factor_zldl_ensemble(A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, alpha[:n_coef], beta[:n_coef]).close()

        t_ens, t_seq, t_factor = stats(ensemble), stats(sequential), stats(factor)
        fz = g.lod_factor_zldl_ensemble(A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, alpha[:n_coef], beta[:n_coef])
        t_solve = stats(lambda: fz.solve_complex(B.data_ptr(), None, ur.data_ptr(), ui.data_ptr(), rhs_members=K, ld_u=F * K))
        zbytes = int(fz.info.bytes)
        fz.close()
        emit({"n_members": K, "n_freq": F, "factor_members": F * K, "chunks": chunks, "members_in_first_chunk": members,
              "ensemble_ms": t_ens, "sequential_ms": t_seq, "ensemble_over_sequential_median": t_ens["median"] / t_seq["median"],
              "factor_ms_first_chunk": t_factor, "solve_ms_first_chunk": t_solve,
              "residual_ms_per_chunk_median": (t_ens["median"] - chunks * (t_factor["median"] + t_solve["median"])) / chunks,
              "launches_ensemble": chunks * (nb + 7 + 1 + 3), "launches_sequential": K * ((F + CHUNK - 1) // CHUNK) * (nb + 7 + 1 + 6),
              "residual_matrix_bytes_per_chunk": 4 * nval * members * 8, "residual_product_bytes_per_chunk": 2 * 4 * nrow * members * 8,
              "factor_bytes_first_chunk": zbytes, "max_rel_residual": float(out["res"].max()), "max_growth": float(out["growth"].max())})


if __name__ == "__main__":
    main()
