// Prints the priority class of every block of a k_solve_tw launch, one number per block: slod_stagger_class of
// csrc/slod_device.h, the function the kernel calls with blockIdx.x and SlodKernelArgs::stagger_row.  Host code only.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -Idealii-slod_amd/csrc tools/dump_stagger_class.cpp -o dump_stagger_class
//   ./dump_stagger_class ROW N_BLOCKS
#include "slod_device.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
  if (argc != 3)
    {
      fprintf(stderr, "usage: %s ROW N_BLOCKS\n", argv[0]);
      return 2;
    }
  const int row = atoi(argv[1]), n = atoi(argv[2]);
  for (int b = 0; b < n; ++b)
    printf("%d\n", slod_stagger_class((unsigned)b, row));
  return 0;
}
