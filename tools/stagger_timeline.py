# Timing experiment: one C2 step of k_solve_tw seen per priority class (diag build, SLOD_DIAG bit 20: clock and HW_ID
# stamps of every workgroup).  Prints the placement check the class rests on (do the blocks b, b + row, b + 2 row, ...
# share a CU?), the phase boundaries per class (class = (block / row) & 3, the row of the balanced launch order), the
# per-CU finish times and how many CUs end on a patch that took the SVD fallback.  SLOD_STAGGER / SLOD_STAGGER_ROW are
# the caller's: run it once with SLOD_STAGGER=0 and once with the mode under test.
import collections
import ctypes as C
import os
import sys

os.environ["SLOD_DIAG"] = str(1 << 20)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("SLOD_LIB_PATH", os.path.join(ROOT, "dealii-slod_amd", "lib", "libslod_hip_diag.so"))
sys.path.insert(0, os.path.join(ROOT, "dealii-slod_amd"))
import numpy as np
import torch
import slod_amd
from slod_amd.synthetic import fill_coefficient

g = slod_amd.Slod(device=0, nref=5, n_sub=8, oversampling=2, spacedim=1, stabilize=1)
dev = torch.device("cuda", 0)
t = torch.from_numpy(fill_coefficient(20250614, "D1e4", g.NE)).to(dev)
g.set_coefficient_device(0, t.data_ptr(), t.numel())
ids = np.arange(g.num_patches, dtype=np.uint32)
plan = g.plan(ids)
b = torch.zeros(len(ids) * plan.stride, dtype=torch.float64, device=dev)
q = torch.zeros_like(b)
for _ in range(3):
    plan.execute(b.data_ptr(), q.data_ptr(), torch.cuda.current_stream().cuda_stream)
torch.cuda.synchronize()
ncm = 25
buf = np.zeros(len(ids) * ncm * ncm)
g.lib.slod_debug_read_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_size_t]
assert g.lib.slod_debug_read_ms(plan.p, buf.ctypes.data_as(C.POINTER(C.c_double)), buf.size) == 0
raw = buf.reshape(len(ids), ncm * ncm)   # row = block of the launch (balanced order), not the caller's patch
n_cu = torch.cuda.get_device_properties(0).multi_processor_count
row = int(os.environ.get("SLOD_STAGGER_ROW", "0")) or n_cu
print("stagger mode %s, row %d, CUs %d, kernel_ms %s" % (os.environ.get("SLOD_STAGGER", "default"), row, n_cu, plan.kernel_ms()))

# placement: CU of a block from HW_ID (CU_ID bits 11:8, SH_ID 12, SE_ID 15:13) and XCC_ID (bits 3:0)
hw = raw[:, 12].astype(np.int64)
xcc = raw[:, 13].astype(np.int64) & 15
cu = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15)
groups = collections.defaultdict(list)
for k in range(len(ids)):
    groups[int(cu[k])].append(k)
sizes = collections.Counter(len(v) for v in groups.values())
as_rows = sum(1 for v in groups.values() if len({k % row for k in v}) == 1 and len({k // row for k in v}) == len(v))
print("placement: %d distinct CUs, workgroups per CU %s; CUs whose blocks are b, b + row, b + 2 row, ...: %d"
      % (len(groups), dict(sizes), as_rows))

us = raw / 100.0
t0 = us[:, 0].min()
cls = (np.arange(len(ids)) // row) & 3
svd = (us[:, 9] - us[:, 8]) > 20.0   # the SVD fallback of the selection stage ran
names = ("start", "prologue", "forward", "meeting", "backward", "select")
cols = (us[:, 0], us[:, 33], us[:, 34], us[:, 35], us[:, 1], us[:, 2])
print("phase ends per class, us after the first start (mean / max):")
for k in range(4):
    m = cls == k
    print("  class %d  n=%3d  fallback patches %3d  " % (k, m.sum(), (svd & m).sum())
          + "  ".join("%s %5.0f/%5.0f" % (nm, (c[m] - t0).mean(), (c[m] - t0).max()) for nm, c in zip(names, cols)))
end = us[:, 2] - t0
fin = np.array([end[v].max() for v in groups.values()])
last = [v[int(np.argmax(end[v]))] for v in groups.values()]
print("per-CU finish (us): mean %.1f  min %.1f  max %.1f;  launch span %.1f" % (fin.mean(), fin.min(), fin.max(), end.max()))
print("CUs that end on a fallback patch: %d of %d;  class of the last patch of a CU: %s"
      % (sum(bool(svd[k]) for k in last), len(groups), dict(collections.Counter(int(cls[k]) for k in last))))
print("fallback patches: %d of %d" % (svd.sum(), len(ids)))
