// Prints the kernel choice (every field of SlodSolveChoice) of slod_choose_solver over a grid of plan
// shapes and tuning knobs, one line per input: the output of two builds of the library can be
// compared with diff.  Host code only, no GPU call is made.
// build + run, from dealii-slod_amd/ after make (the dispatcher calls the sizing functions of the kernel units):
//   hipcc -O1 -std=c++17 --offload-arch=gfx950 -Icsrc ../tools/dump_solver_choice.cpp \
//     $(ls build/*.o | grep -v slod_api) -o build/dump_solver_choice && build/dump_solver_choice > choice.txt
#include "slod_device.h"

#include <algorithm>
#include <cstdio>

int main()
{
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
