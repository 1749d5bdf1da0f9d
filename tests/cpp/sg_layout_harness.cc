// The scratch sizes of the semi-global matchers (bpvo_amd/csrc/kernels_sgm.hip sgm_layout, kernels_sgbm.hip sgbm_layout) without a GPU: linked
// against the product library, whose two functions are plain host code, and printing one size per query of its command line —
// tests/test_sg_layout_cpu.py holds the expectations:
//   sgm ROWS COLS D             -> sgm_scratch_bytes
//   sgbm ROWS COLS MIN_DISP D   -> sgbm_scratch_bytes
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace bpvo_hip {      // (kernels.h, which needs the HIP headers)
size_t sgm_scratch_bytes(int rows, int cols, int ndisp);
size_t sgbm_scratch_bytes(int rows, int cols, int min_disp, int ndisp);
}

int main(int argc, char** argv)
{
  for(int i = 1; i < argc;) {
    if(!std::strcmp(argv[i], "sgm") && i + 3 < argc) {
      std::printf("%zu\n", bpvo_hip::sgm_scratch_bytes(std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3])));
      i += 4;
    } else if(!std::strcmp(argv[i], "sgbm") && i + 4 < argc) {
      std::printf("%zu\n", bpvo_hip::sgbm_scratch_bytes(std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]), std::atoi(argv[i + 4])));
      i += 5;
    } else {
      std::fprintf(stderr, "bad query at argument %d\n", i);
      return 2;
    }
  }
  return 0;
}
