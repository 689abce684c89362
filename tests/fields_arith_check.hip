// fields_arith_check.hip -- runs the device arithmetic of csrc/fields.h for tests/test_fields_arith_paths_gpu.py, which compiles this
// file with hipcc (a second time with -DLF_FP_REDC2 for the two-step REDC branch of fp_mul).
//   fields_arith_check <in.bin> <out.bin>
// in.bin: N records of two elt_t, a and b (a.lo, a.hi, b.lo, b.hi as u64).  out.bin: N records of NOUT elt_t, in this order:
//    0 fp_add(a, b)     1 fp_sub(a, b)     2 fp_mul(a, b)     3 fp_from_mont(a)     4 fp_reduce_limbs(a.lo, a.hi, b.lo, b.hi)
//    5 {f64_add(a.lo, b.lo), f64_add(a.hi, b.hi)}     6 the same with f64_sub     7 the same with f64_mul
//    8 f64x2_add(a, b)     9 f64x2_sub(a, b)     10 f64x2_mul(a, b)     11 f64x2_mul_real(a, b.lo)     12 gf_mul(a, b)
// Every output is written for every record; the test knows which are meaningful (Fp128: a, b < p; F64: all four words below
// 2^64 - 2^32 + 1; gf_mul and fp_reduce_limbs: any words) and checks those against Python integers.  One launch.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../longfellow-zk_amd/csrc/fields.h"

#define NOUT 13

#define CHK(x)                                                                              \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) {                                                                 \
      fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);       \
      exit(2);                                                                              \
    }                                                                                       \
  } while (0)

__global__ void arith(const elt_t* in, elt_t* out, unsigned n) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const elt_t a = ld16(in + 2 * (size_t)i), b = ld16(in + 2 * (size_t)i + 1);
  elt_t* o = out + NOUT * (size_t)i;
  st16(o + 0, fp_add(a, b));
  st16(o + 1, fp_sub(a, b));
  st16(o + 2, fp_mul(a, b));
  st16(o + 3, fp_from_mont(a));
  st16(o + 4, fp_reduce_limbs(a.lo, a.hi, b.lo, b.hi));
  st16(o + 5, elt_t{f64_add(a.lo, b.lo), f64_add(a.hi, b.hi)});
  st16(o + 6, elt_t{f64_sub(a.lo, b.lo), f64_sub(a.hi, b.hi)});
  st16(o + 7, elt_t{f64_mul(a.lo, b.lo), f64_mul(a.hi, b.hi)});
  st16(o + 8, f64x2_add(a, b));
  st16(o + 9, f64x2_sub(a, b));
  st16(o + 10, f64x2_mul(a, b));
  st16(o + 11, f64x2_mul_real(a, b.lo));
  st16(o + 12, gf_mul(a, b));
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
  if (!n || bytes > (1l << 30)) return 2;
  std::vector<elt_t> in(2 * (size_t)n), out(NOUT * (size_t)n);
  if (fread(in.data(), sizeof(elt_t), in.size(), f) != in.size()) return 2;
  fclose(f);
  elt_t *din, *dout;
  CHK(hipMalloc(&din, in.size() * sizeof(elt_t)));
  CHK(hipMalloc(&dout, out.size() * sizeof(elt_t)));
  CHK(hipMemcpy(din, in.data(), in.size() * sizeof(elt_t), hipMemcpyHostToDevice));
  CHK(hipMemset(dout, 0, out.size() * sizeof(elt_t)));
  hipLaunchKernelGGL(arith, dim3((n + 255) / 256), dim3(256), 0, 0, din, dout, n);
  CHK(hipGetLastError());
  CHK(hipDeviceSynchronize());
  CHK(hipMemcpy(out.data(), dout, out.size() * sizeof(elt_t), hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  if (fwrite(out.data(), sizeof(elt_t), out.size(), f) != out.size()) return 2;
  fclose(f);
  printf("records %u\n", n);
  CHK(hipFree(din));
  CHK(hipFree(dout));
  return 0;
}
