// Solver kernel choice (host code): ONE function decides which patch-solve kernel a plan uses,
// with which LDS size and which stages fused in.  slod_plan_create calls it (and rejects the plan
// when nothing fits), slod_plan_execute launches exactly that choice.
#include "slod_device.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

// Tuning knobs of the experiments in tools/ and of the kernel-variant parity tests; read once
// per plan (slod_plan_create), never in the launch path.
//   SLOD_SOLVE=mf|tw|coop|nd  force a kernel family (any other value: the automatic choice)
//   SLOD_FUSE_SELECT=0        selection as its own launch
//   SLOD_FUSE_ASSEMBLE=0      stencil assembly as its own launch
//   SLOD_FUSE_M=0             tw builds M = P^T A^-1 P / H^2 inside its sweeps by default; 0 turns that off and the
//                             selection stage computes M from X again (for A/B timing)
//   SLOD_BWD_KSPLIT=0|1       tw backward sweep (lines of at most three row tiles, nc_max <= 32): K of X = Z - V Y
//                             split between the chain's two waves (default) or, 0, the column-tile split
//   SLOD_SVD_REGS=0|1         SVD fallback of the selection stage (scalar patches of at most 32 columns after the QR): a Jacobi
//                             pair's rows and the pivoted QR's column order live in registers (default) or, 0, the
//                             loops that read them from LDS (what every other patch shape runs; same bits)
//   SLOD_STAGGER=0..4         tw, plans that are resident all at once (scalar problems): wave priorities (s_setprio) by the
//                             class k = (block / row) & 3 of the workgroup, the row of the balanced launch order, so that
//                             the workgroups that share a CU leave the issue-bound forward sweep one after the other.
//                             GJ = Gauss-Jordan waves, H = helpers, "after" = once the meeting line is factorised, before its row
//                             tiles (where the parent set priority 0).
//                               0  GJ 3, H 0, after 0, whatever the class
//                               1  classes 0, 1: GJ 3, H 2, after 2; classes 2, 3: GJ 1, H 0, after 0
//                               2  every wave 3 - k for the whole kernel
//                               3  GJ 3 - k, H max(2 - k, 0), after 0
//                               4  mode 1 with the classes swapped: classes 2, 3 (the rim patches, whose selection stage takes
//                                  the SVD fallback most often and ends last) GJ 3, H 2, after 2; classes 0, 1: GJ 1, H 0, after 0
//   SLOD_STAGGER_ROW=n        blocks per class row (default: the device's CU count, the row of the balanced order)
//   SLOD_TWISTED=0|1 (coop only) SLOD_DEBUG=1 print the choice
//   SLOD_BALANCE=0            launch the patches in the caller's order (default: balanced over the CUs)
SlodTuning slod_read_tuning()
{
  SlodTuning t;
  if (const char *sel = getenv("SLOD_SOLVE"))
    t.solver = !strcmp(sel, "mf") ? SLOD_K_MF : !strcmp(sel, "tw") ? SLOD_K_TW :
               !strcmp(sel, "coop") ? SLOD_K_COOP : !strcmp(sel, "nd") ? SLOD_K_ND : 0;
  if (const char *e = getenv("SLOD_FUSE_SELECT"))
    t.fuse_select = atoi(e) ? 1 : 0;
  if (const char *e = getenv("SLOD_FUSE_ASSEMBLE"))
    t.fuse_assemble = atoi(e) ? 1 : 0;
  if (const char *e = getenv("SLOD_FUSE_M"))
    t.fuse_m = atoi(e) ? 1 : 0;
  if (const char *e = getenv("SLOD_BWD_KSPLIT"))
    t.bwd_ksplit = atoi(e) ? 1 : 0;
  if (const char *e = getenv("SLOD_SVD_REGS"))
    t.svd_regs = atoi(e) ? 1 : 0;
  if (const char *e = getenv("SLOD_STAGGER"))
    t.stagger = std::min(std::max(atoi(e), 0), SLOD_STAGGER_MODES - 1);
  if (const char *e = getenv("SLOD_STAGGER_ROW"))
    t.stagger_row = std::max(atoi(e), 0);
  if (const char *e = getenv("SLOD_TWISTED"))
    t.twisted = atoi(e) ? 1 : 0;
  if (const char *e = getenv("SLOD_BALANCE"))
    t.balance = atoi(e) ? 1 : 0;
  if (const char *e = getenv("SLOD_DEBUG"))
    t.debug = atoi(e) ? 1 : 0;
  return t;
}

// tile size T of the kernels whose Gauss-Jordan wave keeps a line block in registers as an 8 x 8
// lane grid of T x T tiles (k_solve_tw, k_solve_nd): the smallest instantiated T with 8 T >= m_max,
// 0 when the line is too wide
int slod_lane_tile(int m_max)
{
  static const int tiles[] = {2, 3, 4, 5, 6, 8, 10, 12, 14};
  for (int t : tiles)
    if (8 * t >= m_max)
      return t;
  return 0;
}

bool slod_choose_solver(int S, int n_sub, int m_max, int L_max, int nc_max, int nb_buf, int nf_max, size_t n_patches,
                        const SlodTuning &t_in, SlodSolveChoice *out)
{
  const size_t    lds_max = 160 * 1024;
  SlodSolveChoice c;
  const int       nd_nv = slod_solve_nd_cell(S, n_sub, m_max, L_max);
  SlodTuning      t     = t_in;
  if (t.solver == SLOD_K_ND && nd_nv == 0)
    t.solver = 0; // nested dissection does not take this plan (vector problem, cell size): automatic choice
  c.debug = t.debug;
  c.svd_regs = t.svd_regs ? 1 : 0;
  // Kernel families:
  //   tw   twisted + wave-specialised VALU Gauss-Jordan (default: fastest on every BASELINE size,
  //        tools/solver_compare.py)
  //   mf   MFMA-factorised: blocked Gauss-Jordan on the fp64 matrix pipe, twisted, column-tile
  //        private right-hand-side streams (SLOD_SOLVE=mf; automatic only where tw does not fit)
  //   coop all threads cooperate on every pivot (also for tiles narrower than the band)
  const int  wt = slod_lane_tile(m_max);
  const bool lane_tile_fits = wt > 0 && wt >= 2 * S - 1; // the tile is at least as wide as the band
  const auto want = [&](int k) { return t.solver == 0 || t.solver == k; };
  const size_t lds_sel = slod_select_lds_bytes(S, nb_buf, nc_max, nf_max);
  const bool   mf_fits = slod_solve_mf_tiles(S, m_max) > 0 && slod_solve_mf_lds_bytes(S, m_max, nc_max) <= lds_max;
  const bool   tw_fits = lane_tile_fits && slod_solve_tw_lds_bytes(S, m_max, nc_max) <= lds_max;
  if (nd_nv > 0 && t.solver == SLOD_K_ND)
    {
      //   nd   nested dissection: static condensation per cell, edge sets, skeleton lines
      c.kind          = SLOD_K_ND;
      c.nv            = nd_nv;
      c.lds           = slod_solve_nd_lds_bytes(nd_nv, m_max, nc_max);
      c.v_patch_elems = slod_solve_nd_scratch(nd_nv, m_max, L_max, nc_max);
      c.fuse_assemble = t.fuse_assemble ? 1 : 0;
      c.fuse_select   = 0; // 512-thread workgroups: the selection stage is its own launch
    }
  else if (mf_fits && (t.solver == SLOD_K_MF || (t.solver == 0 && !tw_fits && !lane_tile_fits)))
    {
      c.kind          = SLOD_K_MF;
      c.lds           = slod_solve_mf_lds_bytes(S, m_max, nc_max);
      c.v_line_pad    = 16 * slod_solve_mf_tiles(S, m_max);
      c.v_line_elems  = (size_t)c.v_line_pad * c.v_line_pad;
      c.fuse_assemble = (S == 1 && t.fuse_assemble) ? 1 : 0;
      c.fuse_select   = (S == 1 && t.fuse_select && lds_sel <= lds_max) ? 1 : 0;
      if (c.fuse_select && lds_sel > c.lds)
        c.lds = lds_sel;
    }
  else if (want(SLOD_K_TW) && tw_fits)
    {
      c.kind          = SLOD_K_TW;
      c.lds           = slod_solve_tw_lds_bytes(S, m_max, nc_max);
      c.v_line_pad    = 8 * wt;
      c.v_line_elems  = (size_t)64 * wt * wt; // the 8 x 8 lane tiles, both triangles
      c.fuse_assemble = (S == 1 && t.fuse_assemble) ? 1 : 0;
      // the selection stage runs in the same launch (scalar problems) while four workgroups
      // still fit a CU
      c.fuse_select = (S == 1 && t.fuse_select && lds_sel <= 64 * 1024) ? 1 : 0;
      // M from the sweeps (chain tiles of the forward sweep + the meeting line, k_solve_tw; the selection
      // stage, fused or k_select, reads it where the patch allowed it) needs a
      // scalar problem, at most two 16-column tiles and three row tiles per line; its two 16 x 16 LDS
      // tiles must not cost a workgroup per CU (the registers allow at most four)
      if (S == 1 && t.fuse_m != 0 && nc_max <= 32 && 8 * wt <= 48)
        {
          const size_t sel    = c.fuse_select ? lds_sel : 0;
          const size_t with_m = std::max(slod_solve_tw_lds_bytes(S, m_max, nc_max, true), sel);
          if (std::min<size_t>(4, lds_max / with_m) == std::min<size_t>(4, lds_max / std::max(c.lds, sel)))
            {
              c.m_tw = 1;
              c.lds  = slod_solve_tw_lds_bytes(S, m_max, nc_max, true);
            }
        }
      if (c.fuse_select && lds_sel > c.lds)
        c.lds = lds_sel;
      // backward sweep with K split over the chain's two waves: the LDS-resident variant of the loop only
      // (at most three row tiles per line, at most two column tiles)
      c.bwd_ksplit = (t.bwd_ksplit && 8 * wt <= 48 && nc_max <= 32) ? 1 : 0;
    }
  else if (t.solver == 0 || t.solver == SLOD_K_COOP || !lane_tile_fits)
    {
      // twisted (two chains, 512 threads) when the GPU is not full anyway: it halves the
      // dependent chain per patch; one chain per patch otherwise
      int tw = t.twisted >= 0 ? t.twisted : (n_patches < 3 * 256 ? 1 : 0);
      if (slod_solve_lds_bytes(S, m_max, nc_max, tw) > lds_max)
        tw = 0;
      if (slod_solve_lds_bytes(S, m_max, nc_max, tw) > lds_max || (m_max + 15) / 16 > 7)
        return false;
      c.kind       = SLOD_K_COOP;
      c.twisted    = tw;
      c.lds        = slod_solve_lds_bytes(S, m_max, nc_max, tw);
      c.v_line_pad = m_max;
      c.v_line_elems = (size_t)m_max * m_max;
    }
  else
    return false;
  if (!c.fuse_select && lds_sel > lds_max)
    return false; // the stand-alone selection launch does not fit either
  *out = c;
  return true;
}

// Wave priorities by workgroup class (k_solve_tw) need the classes to be co-residents: a plan whose launches
// hold more patches than one resident set (occupancy x CUs; several workspace chunks likewise) starts its
// workgroups one after the other and is de-phased by itself, and its rows do not share CUs.  Vector plans
// stay at 0.  The row is kept whatever the mode: the launch log prints both.
void slod_choose_stagger(int S, const SlodTuning &t, size_t per_launch, int n_cu, SlodSolveChoice *c)
{
  // workgroups per CU: by LDS, and by registers what the launch bounds of k_solve_tw<T,S> ask for (lane_tile_min_waves:
  // 128 VGPRs and four waves per SIMD up to T = 5, two up to T = 7, one beyond; a workgroup puts one wave on each SIMD)
  const int    wt        = c->v_line_pad / 8;
  const size_t by_regs   = wt <= 5 ? 4 : (wt <= 7 ? 2 : 1);
  const size_t occupancy = std::min<size_t>(by_regs, (160 * 1024) / std::max<size_t>(c->lds, 1));
  c->stagger_row = t.stagger_row > 0 ? t.stagger_row : std::max(n_cu, 1);
  // (the four classes are the four co-residents of a CU: a kernel that fits fewer workgroups per CU runs mode 0)
  c->stagger = (c->kind == SLOD_K_TW && S == 1 && occupancy == 4 && per_launch <= occupancy * (size_t)std::max(n_cu, 1)) ? t.stagger : 0;
}

hipError_t slod_launch_solve(int S, const SlodSolveChoice &c, SlodKernelArgs &a, int n_patches, hipStream_t st)
{
  a.m_tw          = c.m_tw;
  a.stagger       = c.stagger;
  a.stagger_row   = c.stagger_row;
  a.bwd_ksplit    = c.bwd_ksplit;
  a.svd_regs      = c.svd_regs;
  a.fuse_select   = c.fuse_select;
  a.fuse_assemble = c.fuse_assemble;
  a.debug         = c.debug;
  switch (c.kind)
    {
      case SLOD_K_MF:
        return slod_launch_solve_mf(S, a, n_patches, c.lds, st);
      case SLOD_K_TW:
        return slod_launch_solve_tw(S, a, n_patches, c.lds, st);
      case SLOD_K_COOP:
        return slod_launch_solve_coop(S, c.twisted, a, n_patches, st);
      case SLOD_K_ND:
        a.nv = c.nv;
        return slod_launch_solve_nd(a, n_patches, c.lds, st);
      default:
        return hipErrorInvalidValue;
    }
}
