// fp_tile_arith_check.hip -- runs the 1024 x 4 tile arithmetic of csrc/fp_tile_arith.h (fpt_mul, fpt_add, fpt_sub) for
// tests/test_fp_tile_arith.py, which compiles this file with hipcc.
//   fp_tile_arith_check <in.bin> <out.bin> <nrand>
// in.bin: N operand pairs (a, b), four u64 each (a.lo, a.hi, b.lo, b.hi), all < p.  out.bin: N triples
// (fpt_mul(a, b), fpt_add(a, b), fpt_sub(a, b)), two u64 each, for the test to check against Python integers.
// Then nrand pseudo-random canonical pairs (a quarter of them with the top 20 bits set) are generated on the device and the
// three routines compared there with fp_mul / fp_add / fp_sub of fields.h; the number of mismatches is printed, and the exit
// status is 0 only if there are none.
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
  const elt_t a = in[2 * i], b = in[2 * i + 1];
  out[3 * i] = fpt_mul(a, b);
  out[3 * i + 1] = fpt_add(a, b);
  out[3 * i + 2] = fpt_sub(a, b);
}

__device__ u64 mix64(u64 z) {  // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ elt_t rand_elt(u64 s) {  // a canonical element; every fourth one with its top 20 bits set
  elt_t x{mix64(s), mix64(s ^ 0x5851F42D4C957F2Dull)};
  if ((s & 3) == 0) x.hi |= FP_P_HI;
  if (x.hi > FP_P_HI || (x.hi == FP_P_HI && x.lo >= FP_P_LO)) {  // x - p < 2^128 - p < p
    const u64 lo = x.lo - FP_P_LO;
    x.hi = x.hi - FP_P_HI - (x.lo < FP_P_LO);
    x.lo = lo;
  }
  return x;
}

__global__ void compare(unsigned long long* bad, unsigned n, u64 seed) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const elt_t a = rand_elt(seed + 2ull * i), b = rand_elt(seed + 2ull * i + 1);
  unsigned nb = 0;
  nb += !elt_eq(fpt_mul(a, b), fp_mul(a, b));
  nb += !elt_eq(fpt_add(a, b), fp_add(a, b));
  nb += !elt_eq(fpt_sub(a, b), fp_sub(a, b));
  if (nb) atomicAdd(bad, (unsigned long long)nb);
}

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s in.bin out.bin nrand\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  const unsigned n = (unsigned)(bytes / (2 * sizeof(elt_t)));
  std::vector<elt_t> in(2 * (size_t)n), out(3 * (size_t)n);
  if (n && fread(in.data(), sizeof(elt_t), in.size(), f) != in.size()) return 2;
  fclose(f);
  elt_t *din, *dout;
  unsigned long long* dbad;
  CHK(hipMalloc(&din, (in.size() + 1) * sizeof(elt_t)));
  CHK(hipMalloc(&dout, (out.size() + 1) * sizeof(elt_t)));
  CHK(hipMalloc(&dbad, sizeof(unsigned long long)));
  CHK(hipMemset(dbad, 0, sizeof(unsigned long long)));
  if (n) {
    CHK(hipMemcpy(din, in.data(), in.size() * sizeof(elt_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(given, dim3((n + 255) / 256), dim3(256), 0, 0, din, dout, n);
    CHK(hipGetLastError());
    CHK(hipMemcpy(out.data(), dout, out.size() * sizeof(elt_t), hipMemcpyDeviceToHost));
  }
  const unsigned nrand = (unsigned)strtoul(argv[3], nullptr, 10);
  if (nrand) {
    hipLaunchKernelGGL(compare, dim3((nrand + 255) / 256), dim3(256), 0, 0, dbad, nrand, 0x243F6A8885A308D3ull);
    CHK(hipGetLastError());
  }
  unsigned long long bad = 0;
  CHK(hipMemcpy(&bad, dbad, sizeof(bad), hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  if (n && fwrite(out.data(), sizeof(elt_t), out.size(), f) != out.size()) return 2;
  fclose(f);
  printf("random pairs %u, mismatches against fields.h %llu\n", nrand, bad);
  CHK(hipFree(din));
  CHK(hipFree(dout));
  CHK(hipFree(dbad));
  return bad == 0 ? 0 : 1;
}
