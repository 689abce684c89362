// fp_tile_full_check.hip -- runs fpt_bfly2_full of csrc/fp_tile_arith.h (two butterflies with full sums, interleaved) next to the
// single routines fpt_add and fpt_sub, with all lanes active and inside a divergent branch, for tests/test_fp128_tile_lean.py,
// which compiles this file with hipcc.  The pattern of fp_tile_pair_check.hip.
//   fp_tile_full_check <in.bin> <out.bin> <n_div>
// in.bin: N operand sets (up, tp, uq, tq), eight u64 each (lo, hi of each), every value < p; N a multiple of 256.
// out.bin: for the lane pattern "all lanes" N records, then for each of the patterns "even lanes", "lane 63" and "lanes 0-31" n_div
// records (the first n_div sets; a multiple of 256, at most N).  A record is RES values of two u64 each:
//   0 - 3  (up + tp, up - tp, uq + tq, uq - tq) by fpt_bfly2_full
//   4      in its low word, bit r set when value r differs from what fpt_add / fpt_sub give in the same lane; the other words MARK
// The records of lanes outside the pattern stay at the sentinel byte 0xa5.  Behind them, for each pattern, one u32 marker per
// record (MARK ^ index), which every lane stores after the branch.
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
constexpr int PATTERNS = 4, RES = 5;

__device__ __forceinline__ bool differ(elt_t a, elt_t b) { return a.lo != b.lo || a.hi != b.hi; }

// n is a multiple of the block size: every wave enters with all 64 lanes active and `on` alone decides who computes
__global__ void given(const elt_t* in, elt_t* out, unsigned* mark, int pattern) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned lane = threadIdx.x & 63;
  const elt_t up = in[4 * i], tp = in[4 * i + 1], uq = in[4 * i + 2], tq = in[4 * i + 3];
  const bool on = pattern == 0 || (pattern == 1 && !(lane & 1)) || (pattern == 2 && lane == 63) || (pattern == 3 && lane < 32);
  if (on) {
    elt_t r[4] = {up, tp, uq, tq};
    fpt_bfly2_full(r[0], r[1], r[2], r[3]);
    const elt_t single[4] = {fpt_add(up, tp), fpt_sub(up, tp), fpt_add(uq, tq), fpt_sub(uq, tq)};
    unsigned bad = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      out[RES * (size_t)i + k] = r[k];
      bad |= differ(r[k], single[k]) ? 1u << k : 0u;
    }
    out[RES * (size_t)i + 4] = elt_t{((u64)MARK << 32) | bad, ((u64)MARK << 32) | MARK};
  }
  mark[i] = MARK ^ i;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s in.bin out.bin n_div\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  const unsigned n = (unsigned)(bytes / (4 * sizeof(elt_t))), n_div = (unsigned)atol(argv[3]);
  if (!n || n % 256 || (long)n * 4 * (long)sizeof(elt_t) != bytes || !n_div || n_div % 256 || n_div > n) return 2;
  std::vector<elt_t> in(4 * (size_t)n), out(RES * (size_t)n);
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
    const unsigned m = pattern == 0 ? n : n_div;
    CHK(hipMemset(dout, 0xa5, RES * (size_t)m * sizeof(elt_t)));
    CHK(hipMemset(dmark, 0, m * sizeof(unsigned)));
    hipLaunchKernelGGL(given, dim3(m / 256), dim3(256), 0, 0, din, dout, dmark, pattern);
    CHK(hipGetLastError());
    CHK(hipMemcpy(out.data(), dout, RES * (size_t)m * sizeof(elt_t), hipMemcpyDeviceToHost));
    CHK(hipMemcpy(mark.data(), dmark, m * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (fwrite(out.data(), sizeof(elt_t), RES * (size_t)m, f) != RES * (size_t)m) return 2;
    marks.insert(marks.end(), mark.begin(), mark.begin() + m);
  }
  if (fwrite(marks.data(), sizeof(unsigned), marks.size(), f) != marks.size()) return 2;
  fclose(f);
  printf("sets %u divergent %u patterns %d\n", n, n_div, PATTERNS);
  CHK(hipFree(din));
  CHK(hipFree(dout));
  CHK(hipFree(dmark));
  return 0;
}
