// fp_tile_lazy_check.hip -- runs the lazy-operand arithmetic of csrc/fp_tile_arith.h (fpt_add_lazy, fpt_sub and fpt_mul with a
// lazy first operand, fpt_canon) for tests/test_fp_tile_lazy.py, which compiles this file with hipcc.
//   fp_tile_lazy_check <in.bin> <out.bin>
// in.bin: N operand pairs (u, t), four u64 each (u.lo, u.hi, t.lo, t.hi); u is any 128-bit value, t < p.  out.bin: N quadruples
// (fpt_add_lazy(u, t), fpt_sub(u, t), fpt_mul(u, t), fpt_canon(u)), two u64 each, for the test to check against Python integers.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
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

__global__ void given(const elt_t* in, elt_t* out, unsigned n) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const elt_t u = in[2 * i], t = in[2 * i + 1];
  out[4 * i] = fpt_add_lazy(u, t);
  out[4 * i + 1] = fpt_sub(u, t);
  out[4 * i + 2] = fpt_mul(u, t);
  out[4 * i + 3] = fpt_canon(u);
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
  if (!n) return 2;
  std::vector<elt_t> in(2 * (size_t)n), out(4 * (size_t)n);
  if (fread(in.data(), sizeof(elt_t), in.size(), f) != in.size()) return 2;
  fclose(f);
  elt_t *din, *dout;
  CHK(hipMalloc(&din, in.size() * sizeof(elt_t)));
  CHK(hipMalloc(&dout, out.size() * sizeof(elt_t)));
  CHK(hipMemcpy(din, in.data(), in.size() * sizeof(elt_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(given, dim3((n + 255) / 256), dim3(256), 0, 0, din, dout, n);
  CHK(hipGetLastError());
  CHK(hipMemcpy(out.data(), dout, out.size() * sizeof(elt_t), hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  if (fwrite(out.data(), sizeof(elt_t), out.size(), f) != out.size()) return 2;
  fclose(f);
  printf("pairs %u\n", n);
  CHK(hipFree(din));
  CHK(hipFree(dout));
  return 0;
}
