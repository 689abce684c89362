// fp_tile_lanes_check.hip -- runs the three routines of csrc/fp_tile_arith.h that end in a conditional +-p (fpt_mul, fpt_sub,
// fpt_add_lazy) with all lanes active and inside a divergent branch, for tests/test_fp_tile_mul50.py, which compiles this file
// with hipcc.
//   fp_tile_lanes_check <in.bin> <out.bin>
// in.bin: N operand sets (u, t), four u64 each (u.lo, u.hi, t.lo, t.hi); u is any 128-bit value, t < p; N a multiple of 256.
// out.bin: for each of the four lane patterns (all lanes, even lanes, lane 63 only, lanes 0-31) N triples
// (fpt_mul(u, t), fpt_sub(u, t), fpt_add_lazy(u, t)), two u64 each, the slots of lanes outside the pattern left at the
// sentinel byte 0xa5; then for each pattern N u32 markers (MARK ^ index), which every lane stores after the branch.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../longfellow-zk_amd/csrc/fp_tile_arith.h"

#define CHK(x)                                                                              \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) {                                                                 \
      fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);       \
      exit(2);                                                                              \
    }                                                                                       \
  } while (0)

constexpr unsigned MARK = 0x5eed0000u;
constexpr int PATTERNS = 4;

// n is a multiple of the block size: every wave enters with all 64 lanes active and `on` alone decides who computes
__global__ void given(const elt_t* in, elt_t* out, unsigned* mark, int pattern) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned lane = threadIdx.x & 63;
  const elt_t u = in[2 * i], t = in[2 * i + 1];
  const bool on = pattern == 0 || (pattern == 1 && !(lane & 1)) || (pattern == 2 && lane == 63) || (pattern == 3 && lane < 32);
  if (on) {
    out[3 * i] = fpt_mul(u, t);
    out[3 * i + 1] = fpt_sub(u, t);
    out[3 * i + 2] = fpt_add_lazy(u, t);
  }
  mark[i] = MARK ^ i;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  const unsigned n = (unsigned)(bytes / (2 * sizeof(elt_t)));
  if (!n || n % 256 || (long)n * 2 * (long)sizeof(elt_t) != bytes) return 2;
  std::vector<elt_t> in(2 * (size_t)n), out(3 * (size_t)n);
  std::vector<unsigned> mark(n);
  if (fread(in.data(), sizeof(elt_t), in.size(), f) != in.size()) return 2;
  fclose(f);
  elt_t *din, *dout;
  unsigned* dmark;
  CHK(hipMalloc(&din, in.size() * sizeof(elt_t)));
  CHK(hipMalloc(&dout, out.size() * sizeof(elt_t)));
  CHK(hipMalloc(&dmark, mark.size() * sizeof(unsigned)));
  CHK(hipMemcpy(din, in.data(), in.size() * sizeof(elt_t), hipMemcpyHostToDevice));
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  std::vector<unsigned> marks;
  for (int pattern = 0; pattern < PATTERNS; pattern++) {
    CHK(hipMemset(dout, 0xa5, out.size() * sizeof(elt_t)));
    CHK(hipMemset(dmark, 0, mark.size() * sizeof(unsigned)));
    hipLaunchKernelGGL(given, dim3(n / 256), dim3(256), 0, 0, din, dout, dmark, pattern);
    CHK(hipGetLastError());
    CHK(hipMemcpy(out.data(), dout, out.size() * sizeof(elt_t), hipMemcpyDeviceToHost));
    CHK(hipMemcpy(mark.data(), dmark, mark.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (fwrite(out.data(), sizeof(elt_t), out.size(), f) != out.size()) return 2;
    marks.insert(marks.end(), mark.begin(), mark.end());
  }
  if (fwrite(marks.data(), sizeof(unsigned), marks.size(), f) != marks.size()) return 2;
  fclose(f);
  printf("sets %u patterns %d\n", n, PATTERNS);
  CHK(hipFree(din));
  CHK(hipFree(dout));
  CHK(hipFree(dmark));
  return 0;
}
