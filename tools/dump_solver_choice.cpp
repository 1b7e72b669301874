// Prints the kernel choice (every field of SlodSolveChoice) of slod_choose_solver over a grid of plan
// shapes and tuning knobs, one line per input: the output of two builds of the library can be
// compared with diff.  Host code only, no GPU call is made.
// With the argument --instantiations it prints instead, for every patch-solve template instantiation of the
// library, whether a plan can reach it -- "auto" (no knob set), "knob" (only with SLOD_SOLVE / SLOD_TWISTED) or
// "never" -- over every plan shape slod_plan_create can derive from a configuration: S, n_sub <= 120, oversampling
// <= 3 and the patch shapes (mx, my) of that oversampling.  The table in DESIGN.md ("Patch-solve instantiations") is
// this output.
// build + run, from dealii-slod_amd/ after make (the dispatcher calls the sizing functions of the kernel units; compile
// and link in two steps, hipcc reads every input of a one-step line as HIP source):
//   hipcc -O1 -std=c++17 --offload-arch=gfx950 -Icsrc -c ../tools/dump_solver_choice.cpp -o build/dump_solver_choice.o
//   hipcc --offload-arch=gfx950 build/dump_solver_choice.o build/slod_dispatch.o build/slod_solve_*.o build/slod_select.o \
//     -o build/dump_solver_choice && build/dump_solver_choice > choice.txt
#include "slod_device.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// the instantiation slod_launch_solve_* picks for a choice (mirrors the switches of the four launchers)
static std::string instantiation(int S, int m_max, const SlodSolveChoice &c)
{
  char b[64];
  switch (c.kind)
    {
      case SLOD_K_TW:
        snprintf(b, sizeof(b), "k_solve_tw<%d,%d>", slod_lane_tile(m_max), S);
        break;
      case SLOD_K_MF:
        snprintf(b, sizeof(b), "k_solve_mf<%d,%d>", slod_solve_mf_tiles(S, m_max), S);
        break;
      case SLOD_K_COOP:
        snprintf(b, sizeof(b), "k_solve<%d,%d,%d>", (m_max + 15) / 16, S, c.twisted);
        break;
      case SLOD_K_ND:
        snprintf(b, sizeof(b), "k_solve_nd<%d,%d>", c.nv, slod_lane_tile(m_max));
        break;
      default:
        snprintf(b, sizeof(b), "?");
    }
  return b;
}

static int dump_instantiations()
{
  // every instantiation the library builds, in the order of the launchers' switches: 0 never, 1 knob, 2 auto
  std::map<std::string, int> reach;
  std::map<std::string, std::string> example;
  std::vector<std::string> order;
  const auto decl = [&](const std::string &n) {
    reach[n] = 0;
    order.push_back(n);
  };
  char      b[64];
  const int tiles[] = {2, 3, 4, 5, 6, 8, 10, 12, 14};
  for (int S = 1; S <= 2; ++S)
    for (int T : tiles)
      snprintf(b, sizeof(b), "k_solve_tw<%d,%d>", T, S), decl(b);
  for (int S = 1; S <= 2; ++S)
    for (int NT = 1; NT <= (S == 1 ? 7 : 5); ++NT)
      snprintf(b, sizeof(b), "k_solve_mf<%d,%d>", NT, S), decl(b);
  for (int S = 1; S <= 2; ++S)
    for (int R = 1; R <= 7; ++R)
      for (int TW = 0; TW <= 1; ++TW)
        snprintf(b, sizeof(b), "k_solve<%d,%d,%d>", R, S, TW), decl(b);
  for (int NV = 4; NV <= 8; NV += 4)
    for (int T = 2; T <= 5; ++T)
      snprintf(b, sizeof(b), "k_solve_nd<%d,%d>", NV, T), decl(b);
  const int solvers[] = {0, SLOD_K_MF, SLOD_K_TW, SLOD_K_COOP, SLOD_K_ND};
  const char *names[] = {"", "mf", "tw", "coop", "nd"};
  for (int S = 1; S <= 2; ++S)
    for (int n_sub = 1; n_sub <= 120; ++n_sub)
      for (int l = 0; l <= 3; ++l)
        for (int a = 1; a <= 2 * l + 1; ++a)   // the shorter side of the plan's widest patch, in cells
          for (int bb = a; bb <= 2 * l + 1; ++bb) // the longer side
            for (int lod = 0; lod <= 1; ++lod)   // LOD patches have no boundary-trace rows
              {
                // the plan sizes as k_make_desc and slod_plan_create derive them
                const int m_max = S * (n_sub * a - 1), L_max = n_sub * bb - 1, nc_max = S * a * bb;
                const int nf_max = S * (n_sub * a + 1) * (n_sub * bb + 1), nb_max = lod ? 0 : S * 2 * n_sub * (a + bb);
                if (m_max < 1 || m_max > 16 * 7 || nc_max > 64)
                  continue; // slod_plan_create rejects these before it asks for a kernel
                const int nb_buf = std::min(nb_max, std::max(S == 1 ? 96 : 80, nc_max + 16));
                for (int n_patches : {1, 64, 1024})
                  for (int si = 0; si < 5; ++si)
                    for (int tw = -1; tw <= 1; ++tw)
                      {
                        SlodTuning t;
                        t.solver  = solvers[si];
                        t.twisted = tw;
                        SlodSolveChoice c;
                        if (!slod_choose_solver(S, n_sub, m_max, L_max, nc_max, nb_buf, nf_max, (size_t)n_patches, t, &c))
                          continue;
                        const std::string name = instantiation(S, m_max, c);
                        if (!reach.count(name))
                          {
                            fprintf(stderr, "not an instantiation of the library: %s\n", name.c_str());
                            return 1;
                          }
                        const int r = (si == 0 && tw == -1) ? 2 : 1;
                        if (r > reach[name])
                          {
                            reach[name] = r;
                            snprintf(b, sizeof(b), "n_sub %d l %d patch %dx%d m_max %d", n_sub, l, a, bb, m_max);
                            example[name] = std::string(b) + (si ? std::string(" SLOD_SOLVE=") + names[si] : std::string()) +
                                            (tw >= 0 ? (tw ? " SLOD_TWISTED=1" : " SLOD_TWISTED=0") : "");
                          }
                      }
              }
  for (const std::string &n : order)
    printf("%-18s %-5s %s\n", n.c_str(), reach[n] == 2 ? "auto" : reach[n] == 1 ? "knob" : "never", example[n].c_str());
  return 0;
}

int main(int argc, char **argv)
{
  if (argc > 1 && !strcmp(argv[1], "--instantiations"))
    return dump_instantiations();
  const int   n_subs[]   = {4, 8, 16};
  const int   nc_maxs[]  = {1, 4, 9, 16, 18, 25, 32, 49, 50, 64};
  const int   patches[]  = {16, 1024};
  const int   solvers[]  = {0, SLOD_K_MF, SLOD_K_TW, SLOD_K_COOP, SLOD_K_ND};
  const char *names[]    = {"auto", "mf", "tw", "coop", "nd"};
  const int   fuse_ms[]  = {-1, 0, 1};
  const auto  kind_name  = [](int k) {
    return k == SLOD_K_MF ? "mf" : k == SLOD_K_TW ? "tw" : k == SLOD_K_COOP ? "coop" : k == SLOD_K_ND ? "nd" : k == 3 ? "ws" : "?";
  };
  for (int S = 1; S <= 2; ++S)
    for (int n_sub : n_subs)
      for (int m_max = 1; m_max <= 112; ++m_max)
        for (int nc_max : nc_maxs)
          for (int n_patches : patches)
            for (int si = 0; si < 5; ++si)
              for (int fuse_m : fuse_ms)
                {
                  // the remaining plan sizes as slod_plan_create derives them for a square patch
                  const int npx = m_max / S + 2, L_max = std::max(1, m_max / S), nf_max = S * npx * npx;
                  const int nb_max = S * 4 * (npx - 1);
                  const int nb_buf = std::min(nb_max, std::max(S == 1 ? 96 : 80, nc_max + 16));
                  SlodTuning t;
                  t.solver = solvers[si];
                  t.fuse_m = fuse_m;
                  SlodSolveChoice c;
                  const bool      ok = slod_choose_solver(S, n_sub, m_max, L_max, nc_max, nb_buf, nf_max, (size_t)n_patches, t, &c);
                  printf("S %d n_sub %2d m_max %3d nc_max %2d n_patches %4d solver %-4s fuse_m %2d : ", S, n_sub, m_max, nc_max,
                         n_patches, names[si], fuse_m);
                  if (!ok)
                    printf("none\n");
                  else
                    printf("kind %-4s lds %6zu fuse_select %d fuse_assemble %d m_tw %d bwd_ksplit %d twisted %d debug %d "
                           "v_line_pad %3d v_line_elems %5zu nv %d v_patch_elems %zu\n",
                           kind_name(c.kind), c.lds, c.fuse_select, c.fuse_assemble, c.m_tw, c.bwd_ksplit, c.twisted, c.debug,
                           c.v_line_pad, c.v_line_elems, c.nv, c.v_patch_elems);
                }
  return 0;
}
