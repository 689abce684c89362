// fp_tile_mul_check.hip -- runs fpt_mul of csrc/fp_tile_arith.h for tests/test_fp_tile_mul_carries.py, which compiles this file
// with hipcc.
//   fp_tile_mul_check <in.bin> <out.bin>
// in.bin: N operand pairs (a, w), four u64 each (a.lo, a.hi, w.lo, w.hi); a is any 128-bit value, w < p (fpt_mul's precondition:
// the carries it does not capture rest on it).  out.bin: N products fpt_mul(a, w), two u64 each, for the test to check against
// Python integers.  One launch.
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

__global__ void products(const elt_t* in, elt_t* out, unsigned n) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = fpt_mul(in[2 * i], in[2 * i + 1]);
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
  std::vector<elt_t> in(2 * (size_t)n), out((size_t)n);
  if (fread(in.data(), sizeof(elt_t), in.size(), f) != in.size()) return 2;
  fclose(f);
  elt_t *din, *dout;
  CHK(hipMalloc(&din, in.size() * sizeof(elt_t)));
  CHK(hipMalloc(&dout, out.size() * sizeof(elt_t)));
  CHK(hipMemcpy(din, in.data(), in.size() * sizeof(elt_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(products, dim3((n + 255) / 256), dim3(256), 0, 0, din, dout, n);
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
