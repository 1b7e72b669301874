// Shared host/device declarations of libslod_hip (not part of the public ABI).
#ifndef SLOD_DEVICE_H
#define SLOD_DEVICE_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// One oversampling patch as the kernels see it.  Produced on the host from the index
// calculus of create_patches()/create_mesh_for_patch() (reference source/LOD.cc:122-244,
// 770-858); nothing in here depends on the coefficient.
struct SlodPatchDesc
{
  int32_t  ox, oy;   // origin of the coefficient tile in the global fine-element grid
  int32_t  nx, ny;   // fine elements per side
  int32_t  mx, my;   // coarse cells per side
  int32_t  ccx, ccy; // centre cell in patch-local cell coordinates (column 0 of P^T)
  int32_t  flags;    // bit0..3: side (L,R,B,T) is on the domain boundary (id 0);
                     // bit4: LOD branch (LOD.cc:563-564); bit5: lines run along y
  int32_t  m, L;     // dofs per grid line, number of interior lines (m <= L)
  int32_t  n_c, n_b; // coarse dofs, id-99 boundary dofs
  int32_t  prob;     // coefficient realisation
  uint32_t plan_index; // position of the patch in the caller's list (diagnostics slot)
  uint64_t out_off;  // offset (doubles) of this patch in basis / premult
};

__host__ __device__ inline size_t slod_mt_stride(int nc_max) { return (size_t)nc_max * nc_max + 1; }

// Priority class of a workgroup of k_solve_tw (SlodKernelArgs::stagger): the blocks b, b + row, b + 2 row, ... of a
// launch that is resident all at once share a CU, and the balanced launch order deals the patches by falling cost
// over rows of `row` blocks -- the row of a block is its rank among its CU's four and its rank by cost.
__host__ __device__ inline int slod_stagger_class(unsigned block, int row) { return (int)((block / (unsigned)(row > 0 ? row : 1)) & 3u); }

enum : int32_t
{
  SLOD_F_LOD        = 1 << 4,
  SLOD_F_TRANSPOSED = 1 << 5
};

// Phase-skip / timeline masks of the timing experiments (tools/): compiled in only with
// -DSLOD_ENABLE_DIAG (lib/libslod_hip_diag.so); the release library has no such branches.
#ifdef SLOD_ENABLE_DIAG
#define SLOD_DG(A, mask) ((A).diag & (mask))
#else
#define SLOD_DG(A, mask) 0
#endif

// Decisions of the SLOD selection stage for one (patch, component): what include/slod.h
// exposes as slod_patch_diag (same layout).
struct SlodPatchDiag
{
  int32_t path;      // 0 LOD branch, 1 SLOD without decisions (QR, proven), 2 SLOD with SVD replay
  int32_t n_cut;     // singular values of G under the 1e-15 cutoff (LOD.cc:667)
  int32_t n_dropped; // triplets removed by the 0.5-loop (LOD.cc:703-725)
  int32_t sweeps;    // Jacobi sweeps of the SVD replay
  double  dinf;      // final ||d||_inf
  double  sigma_max, sigma_min; // extreme singular values of G (path 2), else 0
};

struct SlodKernelArgs
{
  const SlodPatchDesc *desc; // [n_patches of this launch]
  const double        *coef0;
  const double        *coef1;
  size_t               coef_stride; // doubles per problem
  int32_t              NE;          // fine elements per side of the global grid
  int32_t              n_sub;
  int32_t              quirk;       // projection quirk Q2
  int32_t              diag;        // timing experiments (SLOD_ENABLE_DIAG builds only): phase skip mask
  int32_t              debug;       // print the launch configuration (SLOD_DEBUG)
  double               scale;       // h^2/4
  double               invH2;       // 1/H^dim
  // workspace (one slot per patch of the launch)
  double *st;
  size_t  st_stride;
  int32_t nn_max; // node stride inside a stencil slot
  double *vinv;
  size_t  v_stride;
  int32_t m_max;
  int32_t L_max;    // most interior lines of a patch of the plan
  int32_t nv;       // k_solve_nd: cell size of the dissection (fine elements per side)
  double *xs;
  double *zs;       // k_solve_tw: Z of the forward sweep (same strides as xs); other kernels keep Z in xs
  size_t  x_stride;
  int32_t nc_max;
  double *ms;       // per patch nc_max^2 doubles of clock stamps (SLOD_ENABLE_DIAG builds, SLOD_DIAG bit 20); nothing else
  double *mt;       // per patch M built inside the sweeps of k_solve_tw: nc_max^2 doubles, then a flag (1.0: M
                    // is there, 0.0: the patch fell back); stride slod_mt_stride, not the stamps of ms
  int32_t m_tw;     // 1: k_solve_tw builds M in its sweeps where the patch allows it
  int32_t bwd_ksplit; // 1: k_solve_tw splits the backward sweep's GEMM by K half between the chain's two waves
  int32_t stagger;  // k_solve_tw: wave priorities by class of the workgroup (0: Gauss-Jordan waves 3 up to the meeting line,
                    // everything else 0; 1..4: see the knob list of slod_dispatch.cpp)
  int32_t stagger_row; // blocks per row of the balanced launch order: the class is slod_stagger_class(blockIdx.x, stagger_row)
  int32_t svd_regs; // 1: the SVD fallback of the selection stage keeps a Jacobi pair's rows and the pivoted QR's column
                    // order in registers (patches of at most 32 columns; 0: the loops that go through LDS)
  int32_t nb_buf;   // rows of the selection stage's boundary-trace buffer
  int32_t nf_max;   // largest n_fine of the plan
  int32_t fuse_select; // set by slod_launch_solve: the solve kernel also ran the selection stage
  int32_t fuse_assemble; // the solve kernel assembles the stencil of its own patch first
  // outputs
  double  *basis;
  double  *premult;
  int32_t *status;
  SlodPatchDiag *pdiag; // [patches of the PLAN][S], indexed by SlodPatchDesc::plan_index
};

enum SlodSolverKind : int32_t
{
  SLOD_K_MF   = 1, // slod_solve_mf.hip
  SLOD_K_TW   = 2, // slod_solve_tw.hip
  SLOD_K_COOP = 4, // slod_solve_coop.hip
  SLOD_K_ND   = 5  // slod_solve_nd.hip
};

#define SLOD_STAGGER_MODES 5   // 0 .. 4
#define SLOD_STAGGER_DEFAULT 4 // the mode with the lowest median step time at C2
// tuning knobs (environment, read once per plan) and the resulting kernel choice: slod_dispatch.cpp
struct SlodTuning
{
  int solver = 0;        // 0 = automatic, else a SlodSolverKind
  int fuse_select = 1, fuse_assemble = 1, fuse_m = -1; // fuse_m: -1 = the kernel's default
  int twisted = -1;      // coop kernel only: -1 = automatic
  int balance = 1;       // launch order balanced over the CUs (SLOD_BALANCE=0: the caller's order)
  int bwd_ksplit = 1;    // k_solve_tw backward sweep: K split over the chain's two waves (SLOD_BWD_KSPLIT=0: column split)
  int svd_regs = 1;      // selection stage, SVD fallback: Jacobi pairs and the pivot order in registers (SLOD_SVD_REGS=0: LDS loops)
  int stagger = SLOD_STAGGER_DEFAULT; // k_solve_tw: wave priorities by workgroup class (SLOD_STAGGER=0..4; 0: none)
  int stagger_row = 0;   // blocks per class row (SLOD_STAGGER_ROW; 0: the device's CU count, the row of the balanced order)
  int debug = 0;
};
struct SlodSolveChoice
{
  int    kind = 0;
  size_t lds  = 0;
  int    fuse_select = 0, fuse_assemble = 0, m_tw = 0, bwd_ksplit = 0, svd_regs = 0, twisted = 0, debug = 0;
  int    stagger = 0, stagger_row = 1; // set by slod_choose_stagger once the plan's launch size is known
  int    v_line_pad = 0; // rows = columns of a V line as the kernel sees it
  size_t v_line_elems = 0; // doubles per stored V line (k_solve_tw: the 8 x 8 lane tiles, both triangles)
  int    nv = 0;            // k_solve_nd: cell size
  size_t v_patch_elems = 0; // k_solve_nd: doubles of scratch per patch (replaces L_max * v_line_elems)
};
SlodTuning slod_read_tuning();
// the stagger mode of a plan whose launches hold at most `per_launch` patches on a device of n_cu CUs
void       slod_choose_stagger(int S, const SlodTuning &t, size_t per_launch, int n_cu, SlodSolveChoice *c);
bool       slod_choose_solver(int S, int n_sub, int m_max, int L_max, int nc_max, int nb_buf, int nf_max, size_t n_patches,
                              const SlodTuning &t, SlodSolveChoice *out);

// launchers (slod_assemble.hip, slod_solve_{mf,tw,coop,nd}.hip, slod_select.hip)
hipError_t slod_launch_assemble(int S, const SlodKernelArgs &a, int n_patches, hipStream_t st);
hipError_t slod_launch_solve(int S, const SlodSolveChoice &c, SlodKernelArgs &a, int n_patches, hipStream_t st);
hipError_t slod_launch_solve_mf(int S, const SlodKernelArgs &a, int n_patches, size_t lds, hipStream_t st);
hipError_t slod_launch_solve_tw(int S, const SlodKernelArgs &a, int n_patches, size_t lds, hipStream_t st);
hipError_t slod_launch_solve_coop(int S, int twisted, const SlodKernelArgs &a, int n_patches, hipStream_t st);
hipError_t slod_launch_solve_nd(const SlodKernelArgs &a, int n_patches, size_t lds, hipStream_t st);
int        slod_solve_nd_cell(int S, int n_sub, int m_max, int L_max); // cell size, 0 = not applicable
size_t     slod_solve_nd_scratch(int nv, int m_max, int L_max, int nc_max);
size_t     slod_solve_nd_lds_bytes(int nv, int m_max, int nc_max);
hipError_t slod_launch_select(int S, const SlodKernelArgs &a, int n_patches, int nb_max,
                              int nf_max, hipStream_t st);
size_t     slod_solve_lds_bytes(int S, int m_max, int nc_max, int twisted);
size_t     slod_solve_tw_lds_bytes(int S, int m_max, int nc_max, bool with_m = false);
size_t     slod_solve_mf_lds_bytes(int S, int m_max, int nc_max);
int        slod_lane_tile(int m_max); // T: one wave holds a line block as an 8 x 8 lane grid of T x T tiles (m_max <= 8 T), 0 = too wide
int        slod_solve_mf_tiles(int S, int m_max); // 16 x 16 tiles per line side, 0 = does not fit
size_t     slod_select_lds_bytes(int S, int nb_max, int nc_max, int nf_max);

#endif
