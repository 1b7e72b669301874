"""Helpers shared by the GPU test modules (a plain module like fixture_utils.py, not a conftest): handles and
coefficient upload, the parity check of one patch, dense copies of the block rows of the LOD matrices, the fine FEM
reference, the cases (basis, stiffness, mass, pencil) the tests of the LOD-space entry points build on, and the
coefficient fields on which a patch solve must fail (NUMERIC_CONFIGS, _bad_fields), and the random slabs, geometries
and extended-precision references of the slab consumers (SLAB_CONFIGS, _random_slab, _ref_*; pure numpy).  Test
modules import from here and never from each other."""
import numpy as np

from conftest import make_fields

NAN = float("nan")
TOL_PHI = 1e-10
MASS_CONFIGS = {"s1": dict(nref=2, n_sub=2, oversampling=1, spacedim=1),
                "clipped": dict(nref=2, n_sub=4, oversampling=2, spacedim=1),
                "s2": dict(nref=2, n_sub=2, oversampling=1, spacedim=2),
                "rowmajor": dict(n_cells=5, n_sub=3, oversampling=1, spacedim=1)}


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.uint64)


def _mk(so, **kw):
    import slod_amd
    cfg = so.make_cfg(**kw)
    g = slod_amd.Slod(nref=kw.get("nref", 0), n_sub=kw["n_sub"], oversampling=kw["oversampling"],
                      spacedim=kw.get("spacedim", 1), stabilize=kw.get("stabilize", 1),
                      reuse_full=kw.get("reuse_full", 0), proj_quirk=kw.get("proj_quirk", 0),
                      n_cells=kw.get("n_cells", 0))
    return cfg, g


def _upload(g, fields):
    for f, a in enumerate(fields):
        g.set_coefficient(f, a)


def _check_patch(so, cfg, fields, pid, basis, premult, off, label=""):
    p = so.patch_info(cfg, pid)
    s = cfg.spacedim
    phi, psi, _ = so.patch_basis(cfg, fields, pid)
    st = so.assemble_patch(cfg, fields, pid)
    a_inf = np.abs(st).sum(axis=(1, 3)).max()
    n = s * p.n_f
    gphi = basis[off:off + n].reshape(s, p.n_f)
    gpsi = premult[off:off + n].reshape(s, p.n_f)
    ephi = np.abs(gphi - phi).max()
    epsi = np.abs(gpsi - psi).max()
    assert np.isfinite(gphi).all() and np.isfinite(gpsi).all(), label
    assert ephi <= TOL_PHI, "%s patch %d: |dphi| = %.3e" % (label, pid, ephi)
    assert epsi <= TOL_PHI * a_inf, "%s patch %d: |dpsi| = %.3e (tol %.3e)" % (label, pid, epsi, TOL_PHI * a_inf)
    return ephi, epsi / a_inf


def _decisions(g, ids, offs):
    """slod_plan_diagnostics of the same patches (plan path; outputs must equal the host-buffer path)"""
    import torch
    plan = g.plan(ids, offs)
    dev = torch.device("cuda", 0)
    b = torch.zeros(max(plan.output_size, 1), dtype=torch.float64, device=dev)
    q = torch.zeros_like(b)
    plan.execute(b.data_ptr(), q.data_ptr())
    torch.cuda.synchronize()
    plan.status()
    return plan.diagnostics()


def _global_dense(g, cfg_s, basis, premult, stride):
    """Scatter every patch vector to the global fine grid: (N_patches*s) x (NEp^2 * s) dense arrays."""
    s, n, NP = cfg_s, g.cfg.n_subdivisions, g.num_patches
    NEp = g.NE + 1
    Phi = np.zeros((NP * s, NEp * NEp * s))
    Psi = np.zeros_like(Phi)
    for p in range(NP):
        info = g.patch_layout(p)
        nxp, nyp = info.nx + 1, info.ny + 1
        for d in range(s):
            vphi = basis[p * stride + d * info.n_fine:p * stride + (d + 1) * info.n_fine].reshape(nyp, nxp, s)
            vpsi = premult[p * stride + d * info.n_fine:p * stride + (d + 1) * info.n_fine].reshape(nyp, nxp, s)
            G1 = Phi[p * s + d].reshape(NEp, NEp, s)
            G2 = Psi[p * s + d].reshape(NEp, NEp, s)
            G1[info.y0 * n:info.y0 * n + nyp, info.x0 * n:info.x0 * n + nxp, :] = vphi
            G2[info.y0 * n:info.y0 * n + nyp, info.x0 * n:info.x0 * n + nxp, :] = vpsi
    return Phi, Psi


def _rows_to_dense(g, values, cols, s):
    NP, cap = g.num_patches, g.lod_row_capacity()
    A = np.zeros((NP * s, NP * s))
    v = values.reshape(NP, cap, s, s)
    c = cols.reshape(NP, cap)
    for p in range(NP):
        for j in range(cap):
            if c[p, j] != 0xffffffff:
                q = int(c[p, j])
                A[p * s:(p + 1) * s, q * s:(q + 1) * s] = v[p, j]
    return A


def _lod_matrix(g, basis_t, premult_t, stride, s):
    torch, dev = _torch()
    NP, cap = g.num_patches, g.lod_row_capacity()
    values = torch.zeros(NP * cap * s * s, dtype=torch.float64, device=dev)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    g.lod_matrix(np.arange(NP), basis_t.data_ptr(), premult_t.data_ptr(), stride, values.data_ptr(), cols.data_ptr())
    torch.cuda.synchronize()
    return values, cols


def _fem_reference(NE, s, fields, fq=None):
    """Global fine stiffness and load vector with scipy (element matrices of oracle/slod_numpy.py),
    Dirichlet rows/columns removed; returns (A_II, f_I, interior index array)."""
    import scipy.sparse as sp
    import slod_numpy as sn
    NEp = NE + 1
    rows, cols, vals = [], [], []
    f = np.zeros(NEp * NEp * s)
    hf = 1.0 / NE
    g = (sn.G0, sn.G1)
    for ey in range(NE):
        for ex in range(NE):
            ge = (ey * NE + ex) * 4
            K = sn.element_matrix(s, [fld[ge:ge + 4] for fld in fields])
            nodes = [ex + ey * NEp, ex + 1 + ey * NEp, ex + (ey + 1) * NEp, ex + 1 + (ey + 1) * NEp]
            dofs = [nd * s + c for nd in nodes for c in range(s)]
            for i, di in enumerate(dofs):
                for j, dj in enumerate(dofs):
                    rows.append(di), cols.append(dj), vals.append(K[i, j])
            for a, nd in enumerate(nodes):
                for q in range(4):
                    xi, eta = g[q & 1], g[(q >> 1) & 1]
                    N = (xi if a & 1 else 1 - xi) * (eta if a & 2 else 1 - eta)
                    for c in range(s):
                        fv = 1.0 if fq is None else fq[c * NE * NE * 4 + ge + q]
                        f[nd * s + c] += N * fv * hf * hf * 0.25
    A = sp.csr_matrix((vals, (rows, cols)), shape=(NEp * NEp * s, NEp * NEp * s))
    ix, iy = np.meshgrid(np.arange(NEp), np.arange(NEp))
    interior = ((ix > 0) & (ix < NE) & (iy > 0) & (iy < NE)).ravel()
    idx = np.nonzero(np.repeat(interior, s))[0]
    return A[idx][:, idx].tocsc(), f[idx], idx


def _gauss():
    g0 = 0.5 * (1.0 - 1.0 / np.sqrt(3.0))
    return (g0, 1.0 - g0)


def _exact_at_qp(NE):
    """w = sin(pi x) sin(pi y), its gradient and f = 2 pi^2 w at the quadrature points (layout 1)."""
    g = _gauss()
    h = 1.0 / NE
    ey, ex, q = np.meshgrid(np.arange(NE), np.arange(NE), np.arange(4), indexing="ij")
    x = (ex + np.where(q & 1, g[1], g[0])) * h
    y = (ey + np.where(q & 2, g[1], g[0])) * h
    w = np.sin(np.pi * x) * np.sin(np.pi * y)
    wx = np.pi * np.cos(np.pi * x) * np.sin(np.pi * y)
    wy = np.pi * np.sin(np.pi * x) * np.cos(np.pi * y)
    return w.ravel(), np.concatenate([wx.ravel(), wy.ravel()]), (2 * np.pi ** 2 * w).ravel()


def _mass_fine(NE, rho=None):
    """Consistent Q1 mass of the global fine grid, dense [(NE+1)^2]^2, element matrix rho_e h^2/36 [[4,2,2,1],...]."""
    NEp, h = NE + 1, 1.0 / NE
    Me = np.array([[4, 2, 2, 1], [2, 4, 1, 2], [2, 1, 4, 2], [1, 2, 2, 4]], dtype=np.float64) * (h * h / 36.0)
    M = np.zeros((NEp * NEp, NEp * NEp))
    for ey in range(NE):
        for ex in range(NE):
            nodes = np.array([ex + ey * NEp, ex + 1 + ey * NEp, ex + (ey + 1) * NEp, ex + 1 + (ey + 1) * NEp])
            M[np.ix_(nodes, nodes)] += Me * (1.0 if rho is None else rho[ey * NE + ex])
    return M


class _Case:
    pass


# ---- the failure path of the patch solve (test_gpu_numeric_status.py): coefficient fields on which some patch
# matrices are not positive definite, the patches they hit, and a plan run that never raises ----
NUMERIC_CONFIGS = {"scalar": dict(nref=3, n_sub=4, oversampling=1, spacedim=1, stabilize=1),
                   "elasticity": dict(nref=2, n_sub=4, oversampling=1, spacedim=2, stabilize=1)}
# an interior coarse cell: with oversampling 1 the 3 x 3 patch centres around it all exist.  On the scalar grid
# (8 x 8 cells) all nine are full patches, so the cell takes every one of the nine positions in a 3 x 3 patch
BAD_CELL = {"scalar": (3, 3), "elasticity": (1, 1)}
BAD_KINDS = ("negative", "nan", "zero")
BAD_VALUE = {"negative": -1.0, "nan": NAN, "zero": 0.0}
ERR_NUMERIC = -5


def _bad_fields(base, cfg_kw, kind, block=0, cell=None):
    """(fields, bad coarse cells): copies of the base fields [NE][NE][4] with BAD_VALUE[kind] written to every field.
    negative / nan: one 2 x 2 block of fine cells of the coarse cell, fine cells {0,1}^2 (block 0) or {2,3}^2
    (block 1): the fine node in its middle is strictly inside the coarse cell.  zero: every fine cell of the 3 x 3
    coarse cells around the cell (a full patch)."""
    n = cfg_kw["n_sub"]
    N = cfg_kw["n_cells"] if cfg_kw.get("n_cells", 0) > 0 else 1 << cfg_kw["nref"]
    NE = N * n
    cx, cy = cell if cell is not None else BAD_CELL["scalar" if cfg_kw.get("spacedim", 1) == 1 else "elasticity"]
    if kind == "zero":
        assert 1 <= cx < N - 1 and 1 <= cy < N - 1
        x0, x1, y0, y1 = (cx - 1) * n, (cx + 2) * n, (cy - 1) * n, (cy + 2) * n
        cells = {(i, j) for i in range(cx - 1, cx + 2) for j in range(cy - 1, cy + 2)}
    else:
        assert n == 4 and block in (0, 1)
        x0, y0 = cx * n + 2 * block, cy * n + 2 * block
        x1, y1 = x0 + 2, y0 + 2
        cells = {(cx, cy)}
    out = []
    for a in base:
        f = np.array(a, dtype=np.float64).reshape(NE, NE, 4)
        f[y0:y1, x0:x1, :] = BAD_VALUE[kind]
        out.append(f.ravel())
    return out, cells


def _patches_with_cells(so, cfg, cells):
    """Ids of the patches whose extent holds one of the coarse cells (cx, cy), ascending."""
    hit = []
    for pid in range(so.num_patches(cfg)):
        p = so.patch_info(cfg, pid)
        if any(p.x0 <= i < p.x0 + p.mx and p.y0 <= j < p.y0 + p.my for i, j in cells):
            hit.append(pid)
    return hit


def _internal_matrix(so, cfg, fields, pid):
    """Dense A_II of one patch from the oracle's stencil [node][9][s][s], internal dofs in (node, component) order."""
    p, s = so.patch_info(cfg, pid), cfg.spacedim
    st = so.assemble_patch(cfg, fields, pid)
    npx = p.nx + 1
    idx = -np.ones((p.ny + 1, npx), dtype=np.int64)
    idx[1:p.ny, 1:p.nx] = np.arange((p.ny - 1) * (p.nx - 1)).reshape(p.ny - 1, p.nx - 1)
    A = np.zeros((s * (p.nx - 1) * (p.ny - 1),) * 2)
    for iy in range(1, p.ny):
        for ix in range(1, p.nx):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    j = idx[iy + dy, ix + dx]
                    if j >= 0:
                        i = idx[iy, ix]
                        A[i * s:(i + 1) * s, j * s:(j + 1) * s] = st[ix + iy * npx, (dy + 1) * 3 + dx + 1]
    return A


class _BaseOracle:
    """The oracle on the base fields of one NUMERIC_CONFIGS entry, every patch computed once and read-only.  It ignores
    the fields it is handed: a patch that holds no bad cell has the base field's result bit for bit
    (test_bad_fields_hit_exactly_the_patches_with_the_bad_cell), and that is the only kind _check_patch is asked about."""
    _store = {}

    def __init__(self, so, name):
        self._so, self._name = so, name
        self.cfg = so.make_cfg(**NUMERIC_CONFIGS[name])
        self.base = make_fields(so, self.cfg, "D100")

    def __getattr__(self, attr):
        return getattr(self._so, attr)

    def _memo(self, what, pid, fn):
        k = (self._name, what, pid)
        if k not in self._store:
            v = fn()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._store[k] = v
        return self._store[k]

    def patch_basis(self, cfg, fields, pid):
        return self._memo("basis", pid, lambda: self._so.patch_basis(self.cfg, self.base, pid))

    def assemble_patch(self, cfg, fields, pid):
        return self._memo("stencil", pid, lambda: self._so.assemble_patch(self.cfg, self.base, pid))


def _status_of(plan):
    """(code, message) of slod_plan_status: (0, "") when the last execute was fine."""
    import slod_amd
    try:
        plan.status()
    except slod_amd.SlodError as e:
        return e.code, str(e)
    return 0, ""


def _run(plan, stream=None):
    """One execute into fresh NaN-filled slabs (what the plan does not write stays NaN); returns (basis, premult)."""
    torch, dev = _torch()
    b = torch.full((max(plan.output_size, 1),), NAN, dtype=torch.float64, device=dev)
    q = torch.full_like(b, NAN)
    plan.execute(b.data_ptr(), q.data_ptr(), stream)
    return b, q


def _patch_bits(plan, t, k, n):
    """The 64-bit words of the k-th patch of a uniform-stride slab."""
    return _bits(t[k * plan.stride:k * plan.stride + n])


def _build(so, kw, dist="D100", fields=None):
    """Handle, basis slab, premultiplied slab and the stiffness block rows of one configuration."""
    torch, dev = _torch()
    c = _Case()
    c.kw, c.s = kw, kw.get("spacedim", 1)
    cfg, g = _mk(so, stabilize=1, **kw)
    _upload(g, fields if fields is not None else make_fields(so, cfg, dist))
    c.g, c.ids = g, np.arange(g.num_patches, dtype=np.uint32)
    plan = g.plan(c.ids)
    c.stride = plan.stride
    c.b = torch.zeros(len(c.ids) * c.stride, dtype=torch.float64, device=dev)
    c.q = torch.zeros_like(c.b)
    plan.execute(c.b.data_ptr(), c.q.data_ptr())
    plan.status()
    c.values, c.cols = _lod_matrix(g, c.b, c.q, c.stride, c.s)
    c.nrow = g.num_patches * c.s
    return c


def _mass(c, rho_t=None, basis=None):
    torch, dev = _torch()
    NP, cap, s = c.g.num_patches, c.g.lod_row_capacity(), c.s
    values = torch.full((NP * cap * s * s,), NAN, dtype=torch.float64, device=dev)
    cols = torch.zeros(NP * cap, dtype=torch.int32, device=dev)
    c.g.lod_mass_matrix(c.ids, (c.b if basis is None else basis).data_ptr(), c.stride, values.data_ptr(), cols.data_ptr(),
                        d_rho=None if rho_t is None else rho_t.data_ptr())
    torch.cuda.synchronize()
    return values, cols


def _apply(c, values, X, n_rhs, ld_x=None, ld_y=None, first=0):
    torch, dev = _torch()
    ld_y = n_rhs if ld_y is None else ld_y
    Y = torch.full((c.nrow, ld_y), NAN, dtype=torch.float64, device=dev)
    c.g.lod_apply(values.data_ptr(), c.cols.data_ptr(), X.data_ptr() + 8 * first, Y.data_ptr(), n_rhs=n_rhs,
                  ld_x=X.shape[1] if ld_x is None else ld_x, ld_y=ld_y)
    torch.cuda.synchronize()
    return Y


PENCIL_CONFIGS = dict(MASS_CONFIGS,
                      step64=dict(nref=3, n_sub=2, oversampling=1, spacedim=1),   # 64 rows: the cap on the block columns
                      const=dict(nref=2, n_sub=4, oversampling=2, spacedim=1))    # coefficient 1: lambda_2 = lambda_3
_cache = {}


def _symmetrize(c):
    torch, dev = _torch()
    out = torch.full_like(c.values, NAN)
    c.g.lod_matrix_symmetrize(c.values.data_ptr(), c.cols.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out


def _pencil(so, name):
    """Block rows of sym(A_LOD) and M_LOD of one configuration, dense copies, and the dense spectrum; built once."""
    import scipy.linalg as sl
    if name not in _cache:
        c = _build(so, PENCIL_CONFIGS[name], dist="const" if name == "const" else "D100")
        c.mvalues, _ = _mass(c)
        c.sym = _symmetrize(c)
        hc = c.cols.cpu().numpy().view(np.uint32)
        c.A = _rows_to_dense(c.g, c.sym.cpu().numpy(), hc, c.s)
        c.M = _rows_to_dense(c.g, c.mvalues.cpu().numpy(), hc, c.s)
        assert np.array_equal(c.A, c.A.T) and np.array_equal(c.M, c.M.T)
        c.lam, c.vec = sl.eigh(c.A, c.M)                   # vec^T M vec = I
        _cache[name] = c
    return _cache[name]


# ---- slabs that are non-zero on patch rims (test_lod_slab_reference.py on the CPU, test_gpu_lod_slabs.py): geometry as
# plain numbers, random slabs with NaN wherever a consumer must not read, and references of the four slab consumers
# accumulated in np.longdouble.  Nothing here calls the library: the same code takes the extents of a GPU handle
# (g.patch_layout) or of the oracle (so.patch_info). ----
SLAB_CONFIGS = {"golden": dict(nref=2, n_sub=2, oversampling=1, spacedim=2),     # the all-ones geometry of parallel_assembly
                "rowmajor": dict(n_cells=5, n_sub=3, oversampling=1, spacedim=1),   # row-major ids, odd n_sub, odd N
                "wide": dict(nref=2, n_sub=1, oversampling=2, spacedim=2),          # 2 l + 1 > N, a fine element = a coarse cell
                "mixed": dict(nref=3, n_sub=2, oversampling=2, spacedim=1),         # full and clipped patches, pairs sharing a line / nothing
                "whole": dict(n_cells=3, n_sub=2, oversampling=3, spacedim=1)}      # l >= N: every patch is the domain
U53 = 2.0 ** -53
Q1_MASS = np.array([[4, 2, 2, 1], [2, 4, 1, 2], [2, 1, 4, 2], [1, 2, 2, 4]])   # nodes (0,0), (1,0), (0,1), (1,1)
UNUSED = 0xffffffff


def _slab_geometry(N, n, l, s, extents, centres):
    """Per patch the extent (x0, y0, mx, my) in coarse cells, the centre cell, the node count (mx n + 1)(my n + 1) and
    n_fine = s * nodes, the words of one of its s vectors ([node][component], nodes lexicographic, x fastest)."""
    geom = _Case()
    geom.N, geom.n, geom.l, geom.s = N, n, l, s
    geom.NE, geom.NEp = N * n, N * n + 1
    geom.ext = np.array(extents, dtype=np.int64).reshape(-1, 4)
    geom.centres = np.array(centres, dtype=np.int64).reshape(-1, 2)
    geom.NP = len(geom.ext)
    assert geom.NP == N * N == len(geom.centres)
    geom.nnode = (geom.ext[:, 2] * n + 1) * (geom.ext[:, 3] * n + 1)
    geom.n_fine = s * geom.nnode
    geom.span = 4 * l + 3
    geom.cap = geom.span ** 2
    geom.field = geom.NEp * geom.NEp * s
    geom.pid = {(int(x), int(y)): p for p, (x, y) in enumerate(geom.centres)}
    assert len(geom.pid) == geom.NP
    return geom


def _layout_geometry(kw, layout):
    """_slab_geometry of one configuration; layout(p) has x0, y0, mx, my, cx, cy (g.patch_layout or so.patch_info)."""
    N = kw["n_cells"] if kw.get("n_cells", 0) > 0 else 1 << kw["nref"]
    infos = [layout(p) for p in range(N * N)]
    return _slab_geometry(N, kw["n_sub"], kw["oversampling"], kw.get("spacedim", 1), [(i.x0, i.y0, i.mx, i.my) for i in infos],
                          [(i.cx, i.cy) for i in infos])


def _rim_mask(ny, nx):
    rim = np.zeros((ny, nx), dtype=bool)
    rim[0, :] = rim[-1, :] = rim[:, 0] = rim[:, -1] = True
    return rim


def _random_slab(geom, stride, seed, members=1, member_gap=0):
    """(slab, vecs): vecs[k][p][d, iy, ix, c], every word uniform in [-1, 1] and none 0 on a rim; the values depend on
    the seed alone, not on the stride.  slab: member k from k (NP stride + member_gap), patch p at + p stride, NaN in
    every word between s n_fine(p) and the stride and between the members."""
    s, n = geom.s, geom.n
    assert stride >= s * geom.n_fine.max()
    rng = np.random.default_rng(seed)
    mstride = geom.NP * stride + member_gap
    slab = np.full(members * mstride, NAN)
    vecs = []
    for k in range(members):
        vecs.append([])
        for p in range(geom.NP):
            nx, ny = geom.ext[p, 2] * n + 1, geom.ext[p, 3] * n + 1
            v = rng.uniform(-1.0, 1.0, (s, ny, nx, s))
            assert (v[:, _rim_mask(ny, nx), :] != 0.0).all()
            vecs[k].append(v)
            off = k * mstride + p * stride
            slab[off:off + v.size] = v.ravel()
    assert np.isfinite(slab).sum() == members * s * geom.n_fine.sum()
    return slab, vecs


def _overlap(geom, p, q):
    """The closed rectangles of p and q in global fine nodes: (xa, xb, ya, yb) inclusive, or None when they do not meet."""
    n = geom.n
    px0, py0, pmx, pmy = geom.ext[p]
    qx0, qy0, qmx, qmy = geom.ext[q]
    xa, xb = max(px0, qx0) * n, min(px0 + pmx, qx0 + qmx) * n
    ya, yb = max(py0, qy0) * n, min(py0 + pmy, qy0 + qmy) * n
    return None if xa > xb or ya > yb else (xa, xb, ya, yb)


def _window(geom, v, p, rect):
    """The nodes of rect of the vectors v[d, iy, ix, c] of patch p, in extended precision."""
    xa, xb, ya, yb = rect
    ox, oy = geom.ext[p, 0] * geom.n, geom.ext[p, 1] * geom.n
    return v[:, ya - oy:yb - oy + 1, xa - ox:xb - ox + 1, :].astype(np.longdouble)


def _ref_matrix(geom, Phi, Psi):
    """A[(p,d),(q,e)] = sum over the shared nodes i and the components c of phi_{p,d}(i,c) psi_{q,e}(i,c).  Returns
    (ref, S_abs, m, shared): [NP][NP][s][s] values, the same sums over absolute values, the number of products per entry
    [NP][NP], and the pattern [NP][NP] (closed rectangles intersect)."""
    NP, s = geom.NP, geom.s
    ref = np.zeros((NP, NP, s, s), dtype=np.longdouble)
    sabs = np.zeros_like(ref)
    m = np.zeros((NP, NP), dtype=np.int64)
    shared = np.zeros((NP, NP), dtype=bool)
    for p in range(NP):
        for q in range(NP):
            rect = _overlap(geom, p, q)
            if rect is None:
                continue
            shared[p, q] = True
            a, b = _window(geom, Phi[p], p, rect), _window(geom, Psi[q], q, rect)
            ref[p, q] = (a[:, None] * b[None, :]).sum(axis=(2, 3, 4))
            sabs[p, q] = (np.abs(a)[:, None] * np.abs(b)[None, :]).sum(axis=(2, 3, 4))
            m[p, q] = a[0].size
    return ref, sabs, m, shared


def _ref_mass(geom, Phi, rho=None):
    """M[(p,d),(q,e)] = sum over the fine elements E of the intersection rectangle and the components c of
    rho_E h^2 / 36  a^T Q1_MASS b,  a, b the corner values of phi_{p,d}(., c) and phi_{q,e}(., c) on E; rho [NE][NE], None = 1.
    Returns (ref, S_abs, m, shared) as _ref_matrix, m = elements x components (the roundings inside one element form
    are the + 16 of the bar); a pair that shares only a line has ref = S_abs = m = 0."""
    NP, s, NE = geom.NP, geom.s, geom.NE
    ref = np.zeros((NP, NP, s, s), dtype=np.longdouble)
    sabs = np.zeros_like(ref)
    m = np.zeros((NP, NP), dtype=np.int64)
    shared = np.zeros((NP, NP), dtype=bool)
    scale = (np.longdouble(1) / np.longdouble(NE)) ** 2 / np.longdouble(36)
    r_all = np.ones((NE, NE), dtype=np.longdouble) if rho is None else np.asarray(rho).reshape(NE, NE).astype(np.longdouble)

    def corners(v):
        return [v[:, :-1, :-1], v[:, :-1, 1:], v[:, 1:, :-1], v[:, 1:, 1:]]

    for p in range(NP):
        for q in range(NP):
            rect = _overlap(geom, p, q)
            if rect is None:
                continue
            shared[p, q] = True
            xa, xb, ya, yb = rect
            if xa == xb or ya == yb:
                continue
            a, b = corners(_window(geom, Phi[p], p, rect)), corners(_window(geom, Phi[q], q, rect))
            r = r_all[ya:yb, xa:xb][None, None, :, :, None]
            for i in range(4):
                mb = sum(int(Q1_MASS[i, j]) * b[j] for j in range(4))
                mb_abs = sum(int(Q1_MASS[i, j]) * np.abs(b[j]) for j in range(4))
                ref[p, q] += (a[i][:, None] * mb[None, :] * r).sum(axis=(2, 3, 4))
                sabs[p, q] += (np.abs(a[i])[:, None] * mb_abs[None, :] * r).sum(axis=(2, 3, 4))
            ref[p, q] *= scale
            sabs[p, q] *= scale
            m[p, q] = (xb - xa) * (yb - ya) * s
    return ref, sabs, m, shared


def _ref_rhs(geom, Phi, F):
    """(C^T f)[p s + d] = sum over every node i of patch p and the components c of phi_{p,d}(i,c) f(i,c); F [NEp][NEp][s].
    Returns (ref, S_abs, m), each [NP s]."""
    NP, s, n = geom.NP, geom.s, geom.n
    F = np.asarray(F).reshape(geom.NEp, geom.NEp, s).astype(np.longdouble)
    ref = np.zeros(NP * s, dtype=np.longdouble)
    sabs = np.zeros_like(ref)
    m = np.zeros(NP * s, dtype=np.int64)
    for p in range(NP):
        x0, y0, mx, my = geom.ext[p]
        f = F[y0 * n:(y0 + my) * n + 1, x0 * n:(x0 + mx) * n + 1, :]
        v = Phi[p].astype(np.longdouble)
        ref[p * s:(p + 1) * s] = (v * f[None]).sum(axis=(1, 2, 3))
        sabs[p * s:(p + 1) * s] = (np.abs(v) * np.abs(f)[None]).sum(axis=(1, 2, 3))
        m[p * s:(p + 1) * s] = f.size
    return ref, sabs, m


def _ref_reconstruct(geom, Phi, U):
    """(C u)(i, c) = sum over every patch p that covers the node i and its vectors d of phi_{p,d}(i,c) u[p s + d].
    Returns (ref, S_abs, m), each [NEp][NEp][s]."""
    NP, s, n = geom.NP, geom.s, geom.n
    U = np.asarray(U).reshape(NP, s).astype(np.longdouble)
    ref = np.zeros((geom.NEp, geom.NEp, s), dtype=np.longdouble)
    sabs = np.zeros_like(ref)
    m = np.zeros((geom.NEp, geom.NEp, s), dtype=np.int64)
    for p in range(NP):
        x0, y0, mx, my = geom.ext[p]
        win = (slice(y0 * n, (y0 + my) * n + 1), slice(x0 * n, (x0 + mx) * n + 1))
        v = Phi[p].astype(np.longdouble)
        for d in range(s):
            ref[win] += v[d] * U[p, d]
            sabs[win] += np.abs(v[d]) * np.abs(U[p, d])
            m[win] += 1
    return ref, sabs, m


def _slab_bar(got, ref, sabs, m):
    """The one bar of every value comparison: |got - ref| <= (m + 16) 2^-53 S_abs, the bound of a sum of m products in
    any order (Higham, Accuracy and Stability, sections 3.1 and 4.2) plus the 16 roundings inside one term.  Returns
    (ok, worst |got - ref| / bound); where the bound is 0 the value must be the reference exactly."""
    err = np.abs(np.asarray(got).astype(np.longdouble) - ref)
    bound = (np.asarray(m).astype(np.longdouble) + 16) * np.longdouble(U53) * sabs
    ok = bool((err <= bound).all())
    pos = bound > 0
    return ok, float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def _slot_columns(geom, shared):
    """cols[p][j] of a block row from the pattern alone: slot j of row p is the patch whose centre cell lies at
    (j % span, j / span) - span / 2 from p's (include/slod.h), UNUSED when there is none or the two share no node."""
    cols = np.full((geom.NP, geom.cap), UNUSED, dtype=np.uint32)
    for p in range(geom.NP):
        cx, cy = geom.centres[p]
        for j in range(geom.cap):
            q = geom.pid.get((int(cx) + j % geom.span - geom.span // 2, int(cy) + j // geom.span - geom.span // 2))
            if q is not None and shared[p, q]:
                cols[p, j] = q
    assert ((cols != UNUSED).sum(axis=1) == shared.sum(axis=1)).all()   # every coupled patch has a slot
    return cols


def _blocks_by_column(geom, values, cols):
    """[NP][NP][s][s] copy of block rows [NP][cap][s][s]; unused slots are left out."""
    s = geom.s
    v = np.asarray(values).reshape(geom.NP, geom.cap, s, s)
    out = np.zeros((geom.NP, geom.NP, s, s))
    used = np.asarray(cols).reshape(geom.NP, geom.cap) != UNUSED
    rows = np.repeat(np.arange(geom.NP), geom.cap).reshape(geom.NP, geom.cap)
    out[rows[used], np.asarray(cols).reshape(geom.NP, geom.cap)[used].astype(np.int64)] = v[used]
    return out
