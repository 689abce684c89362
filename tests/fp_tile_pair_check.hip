// fp_tile_pair_check.hip -- runs the paired routines of csrc/fp_tile_arith.h (fpt_mul2_t<false>, fpt_mul2_t<true>, fpt_bfly2_lazy,
// fpt_bfly_lazy, fpt_canon2) next to the single ones, with all lanes active and inside a divergent branch, for
// tests/test_fp_tile_pairs.py, which compiles this file with hipcc.
//   fp_tile_pair_check <in.bin> <out.bin> <n_div>
// in.bin: N operand sets (up, tp, uq, tq), eight u64 each (lo, hi of each); u is any 128-bit value, t < p; N a multiple of 256.
// The uniform twiddles of fpt_mul2_t<true> are tp and tq of the first set of the wave (sets 64 w .. 64 w + 63 are one wave).
// out.bin: for the lane pattern "all lanes" N records, then for each of the patterns "even lanes", "lane 63" and "lanes 0-31" n_div
// records (the first n_div sets; a multiple of 256, at most N).  A record is RES values of two u64 each:
//   0, 1   up tp, uq tq by fpt_mul2_t<false>        2, 3   up tp', uq tq' by fpt_mul2_t<true> (tp', tq' the wave's)
//   4 - 7  (up + tp lazy, up - tp, uq + tq lazy, uq - tq) by fpt_bfly2_lazy        8, 9   (up + tp lazy, up - tp) by fpt_bfly_lazy
//   10, 11 up, uq canonical by fpt_canon2
//   12     in its low word, bit r set when value r differs from what the single routines give in the same lane (fpt_mul, fpt_mul_sw,
//          fpt_add_lazy, fpt_sub, fpt_canon); the other words MARK
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
constexpr int PATTERNS = 4, RES = 13;

__device__ __forceinline__ bool differ(elt_t a, elt_t b) { return a.lo != b.lo || a.hi != b.hi; }
__device__ __forceinline__ elt_t uniform(elt_t a) {  // the value of the first active lane, in SGPRs
  const u32 w0 = __builtin_amdgcn_readfirstlane((u32)a.lo), w1 = __builtin_amdgcn_readfirstlane((u32)(a.lo >> 32)),
            w2 = __builtin_amdgcn_readfirstlane((u32)a.hi), w3 = __builtin_amdgcn_readfirstlane((u32)(a.hi >> 32));
  return elt_t{((u64)w1 << 32) | w0, ((u64)w3 << 32) | w2};
}

// n is a multiple of the block size: every wave enters with all 64 lanes active and `on` alone decides who computes
__global__ void given(const elt_t* in, elt_t* out, unsigned* mark, int pattern) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned lane = threadIdx.x & 63, first = i & ~63u;
  const elt_t up = in[4 * i], tp = in[4 * i + 1], uq = in[4 * i + 2], tq = in[4 * i + 3];
  const elt_t wp = uniform(in[4 * first + 1]), wq = uniform(in[4 * first + 3]);  // read with all lanes active: the same in every lane
  const bool on = pattern == 0 || (pattern == 1 && !(lane & 1)) || (pattern == 2 && lane == 63) || (pattern == 3 && lane < 32);
  if (on) {
    elt_t r[12];
    r[0] = up, r[1] = uq;
    fpt_mul2(r[0], tp, r[1], tq);
    r[2] = up, r[3] = uq;
    fpt_mul2_sw(r[2], wp, r[3], wq);
    r[4] = up, r[5] = tp, r[6] = uq, r[7] = tq;
    fpt_bfly2_lazy(r[4], r[5], r[6], r[7]);
    r[8] = up, r[9] = tp;
    fpt_bfly_lazy(r[8], r[9]);
    r[10] = up, r[11] = uq;
    fpt_canon2(r[10], r[11]);
    const elt_t single[12] = {fpt_mul(up, tp),    fpt_mul(uq, tq), fpt_mul_sw(up, wp),   fpt_mul_sw(uq, wq), fpt_add_lazy(up, tp), fpt_sub(up, tp),
                              fpt_add_lazy(uq, tq), fpt_sub(uq, tq), fpt_add_lazy(up, tp), fpt_sub(up, tp),    fpt_canon(up),        fpt_canon(uq)};
    unsigned bad = 0;
#pragma unroll
    for (int k = 0; k < 12; k++) {
      out[RES * (size_t)i + k] = r[k];
      bad |= differ(r[k], single[k]) ? 1u << k : 0u;
    }
    out[RES * (size_t)i + 12] = elt_t{((u64)MARK << 32) | bad, ((u64)MARK << 32) | MARK};
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
