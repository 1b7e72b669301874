#!/usr/bin/env python3
"""Time the refresh after a local coefficient change against the full path on BASELINE configuration C2 (2-D Poisson,
H = 1/32, n_sub 8, oversampling 2: 1024 patches, 121 slots per block row), coefficient D1e4, in one process.

The change: the fine elements of ONE coarse cell (default the cell (16, 16)) are scaled by 2 and, on the next
repetition, scaled back, so that every repetition sees the same dirty set.  Per step, medians of --reps after a warm-up,
host wall time around a synchronised call sequence (plan creation is host work, so events alone would miss it):
  refresh   slod_update_coefficient (device data) + slod_plan_create_dirty + its execute + slod_lod_matrix_update,
            in place on the slab and the matrix of the old build;
  full      the entry points a caller had before: slod_set_coefficient (device data) + slod_plan_create over all
            patches + its execute + slod_lod_matrix on all rows.  A caller that keeps its full plan pays the line
            full_keeping_the_plan_ms instead (no plan creation).
The refreshed slab and matrix are compared with the full rebuild word for word once, before the timing.  One JSON line.

  python tools/lod_update_timing.py [--reps 7] [--cell 16 16]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cell", type=int, nargs=2, default=[16, 16])
    args = ap.parse_args()
    import torch
    import slod_amd
    from slod_amd.synthetic import fill_coefficient
    if not torch.cuda.is_available():
        raise SystemExit("lod_update_timing.py needs an MI355X: no HIP device visible (no CPU fallback)")
    dev = torch.device("cuda", 0)
    g = slod_amd.Slod(**C2)
    NP, cap, NE, n = g.num_patches, g.lod_row_capacity(), g.NE, C2["n_sub"]
    base = fill_coefficient(SEED, "D1e4", NE).reshape(NE, NE, 4)
    other = base.copy()
    cx, cy = args.cell
    other[cy * n:(cy + 1) * n, cx * n:(cx + 1) * n, :] *= 2.0
    fields = [torch.from_numpy(a.ravel()).to(dev) for a in (base, other)]
    ids = np.arange(NP, dtype=np.uint32)
    g.set_coefficient_device(0, fields[0].data_ptr(), fields[0].numel())
    full_plan = g.plan(ids)
    stride = full_plan.stride
    b = torch.zeros(NP * stride, dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    values = torch.zeros(NP * cap, dtype=torch.float64, device=dev)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    dirty = torch.zeros(NP, dtype=torch.int32, device=dev)
    bf, qf, vf, cf = torch.zeros_like(b), torch.zeros_like(q), torch.zeros_like(values), torch.zeros_like(cols)

    def full(field, plan=None, out=(bf, qf, vf, cf)):
        g.set_coefficient_device(0, field.data_ptr(), field.numel())
        p = plan if plan is not None else g.plan(ids)
        p.execute(out[0].data_ptr(), out[1].data_ptr())
        p.status()
        g.lod_matrix(ids, out[0].data_ptr(), out[1].data_ptr(), stride, out[2].data_ptr(), out[3].data_ptr())
        torch.cuda.synchronize()
        if plan is None:
            p.close()

    info = {}

    def refresh(field, parts=None):
        t = [time.perf_counter()]

        def lap():
            torch.cuda.synchronize()
            t.append(time.perf_counter())

        dirty.zero_()
        torch.cuda.synchronize()
        t[0] = time.perf_counter()
        g.update_coefficient_device(0, field.data_ptr(), field.numel(), dirty.data_ptr())
        lap()
        p = g.plan_dirty(dirty.data_ptr())
        lap()
        p.execute(b.data_ptr(), q.data_ptr())
        p.status()
        lap()
        g.lod_matrix_update(dirty.data_ptr(), b.data_ptr(), q.data_ptr(), stride, values.data_ptr())
        lap()
        info["dirty"] = len(p.gids)
        p.close()
        if parts is not None:
            parts.append([(t[i + 1] - t[i]) * 1e3 for i in range(4)])

    # the old build, one refresh, and the word-for-word comparison with a full rebuild
    full(fields[0], full_plan, (b, q, values, cols))
    refresh(fields[1])
    full(fields[1], full_plan)
    bits = lambda x: x.cpu().numpy().view(np.uint64 if x.dtype == torch.float64 else np.uint32)
    slab_equal = bool(np.array_equal(bits(b), bits(bf)) and np.array_equal(bits(q), bits(qf)))
    matrix_equal = bool(np.array_equal(bits(values), bits(vf)))
    hc, f = bits(cols).reshape(NP, cap), bits(dirty) != 0
    used = hc != 0xffffffff
    recomputed = int((used & (f[:, None] | f[np.where(used, hc, 0)])).sum())

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def median(xs):
        return sorted(xs)[len(xs) // 2]

    # every repetition changes the coefficient: the fields alternate, starting from the one that is not stored
    parts, t_refresh, t_full, t_keep = [], [], [], []
    refresh(fields[0])                                                     # warm-up; fields[0] is stored now
    for r in range(args.reps):
        t_refresh.append(wall(lambda: refresh(fields[(r + 1) % 2], parts)))
    full(fields[0])
    for r in range(args.reps):
        t_full.append(wall(lambda: full(fields[(r + 1) % 2])))
    for r in range(args.reps):
        t_keep.append(wall(lambda: full(fields[(r + 1) % 2], full_plan)))
    names = ("update_coefficient_ms", "dirty_plan_create_ms", "dirty_plan_execute_ms", "matrix_update_ms")
    out = {"config": "C2", "cell": [cx, cy], "patches": NP, "dirty_patches": info["dirty"], "used_entries": int(used.sum()),
           "entries_recomputed": recomputed, "refreshed_slab_equals_full_rebuild": slab_equal,
           "refreshed_matrix_equals_full_rebuild": matrix_equal, "reps": args.reps,
           "refresh_ms": median(t_refresh), "full_ms": median(t_full), "full_keeping_the_plan_ms": median(t_keep),
           "speedup": median(t_full) / median(t_refresh), "speedup_keeping_the_plan": median(t_keep) / median(t_refresh)}
    for i, name in enumerate(names):
        out[name] = median([p[i] for p in parts])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
