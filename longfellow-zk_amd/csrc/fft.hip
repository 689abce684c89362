// fft.hip -- K1 (Fp128 radix-2 FFT) and K2 (GF(2^128) LCH14 additive FFT).
//
// Both transforms are run as one or two "tile passes".  A pass gives each
// workgroup a tile of T points x C batch columns (T*C <= 8192 elements = 128 KiB
// of the CU's 160 KiB LDS), runs log2(T) butterfly stages entirely in LDS and
// writes the tile back once, so HBM sees one read + one write per pass:
//   n <= 8192 : one pass, batch = rows
//   n  > 8192 : n = n1 * n2 (n2 = 1024).  Pass A: n1-point transforms down the
//               strided dimension (C consecutive columns per tile => coalesced
//               C*16-byte segments), pass B: n2-point transforms on contiguous rows.
// Reference: lib/algebra/fft.h:70-201 (Fp128), lib/gf2k/lch14.h:92-144 (LCH14).
#include <string>
#include <type_traits>

#include "ctx.h"
#include "fp_tile_arith.h"

int lf_lch14_fft_bitsliced(lfgpu_ctx* c, int k, int inverse, size_t rows, unsigned l, u64 coset, void* d_B, size_t ld);

#define TILE_ELTS 8192u  // largest tile (128 KiB)
// Tile geometry: 2^13 elements / 1024 threads (one workgroup per CU) or 2^12 elements / 512 threads
// (two workgroups per CU, so one workgroup's HBM phase overlaps the other's butterfly phase).
// c->tile_log = 12 by default: measured 46.9 ms vs 54.8 ms per 2^20 x 1024 Fp128 batch (profiles/r01)

struct TilePlan {
  const elt_t* src;
  elt_t* dst;
  long long src_row, dst_row;    // grid.y (row) strides, elements
  long long src_tile, dst_tile;  // grid.x (tile) strides
  long long sk, sc, dk, dc;      // strides of the point index k and batch index c
  u32 logT, logC, nbatch;        // nbatch: total batch columns over all tiles (bounds)
  u32 kfast_src, kfast_dst;      // 1: consecutive lanes walk k (stride-1 side), 0: walk c
  u32 wlds;                      // Fp128: stage twiddles staged in LDS behind the tile
};

__device__ __forceinline__ u32 bitrev(u32 x, u32 bits) { return bits ? (__brev(x) >> (32 - bits)) : 0; }

// LDS slot of point k, column c.  Rows are C*16 bytes; bit-reversed / strided row indices would put
// the 8 lanes of one ds_write_b128 pass on the same banks, so the top four bits of k are XORed into
// the low slot bits (a bijection inside every aligned 16-slot = 256-byte bank row).
__device__ __forceinline__ u32 lds_slot(u32 k, u32 c, u32 logT, u32 logC) {
  u32 slot = (k << logC) + c;
  if (logT >= 8 && logC >= 3) slot ^= (k >> (logT - 4)) & 15u;
  return slot;
}

// ------------------------------------------------------------------ K1: Fp128 (and the F64_2 of the reference's FFT tests)
// What K1 needs of a field with 16-byte elements: add, sub, the product with a twiddle (a power of the root) and, on the
// host, the general product, 1 and the inverse.  Fp128 is the field of the prover; F64_2 = Fp2<Fp<1>> over
// p = 2^64 - 2^32 + 1 is the second field of lib/algebra/fft_test.cc:205-229 (BM_FFT_F64_2) -- same plan, same kernel.
struct Fp128Ops {
  static constexpr const char* kKey = "fp";
  static LF_HD elt_t add(elt_t a, elt_t b) { return fp_add(a, b); }
  static LF_HD elt_t sub(elt_t a, elt_t b) { return fp_sub(a, b); }
  static LF_HD elt_t mul_tw(elt_t a, elt_t w) { return fp_mul(a, w); }
  static elt_t hmul(elt_t a, elt_t b) { return fp_mul(a, b); }
  static elt_t one() { return h_fp_of_scalar(1); }
  static elt_t inv(elt_t a) { return h_fp_inv(a); }
};
static u64 h_f64_pow(u64 x, u64 e) {
  u64 r = 0xFFFFFFFFull;  // 2^64 mod p: the Montgomery image of 1
  for (; e; e >>= 1) {
    if (e & 1) r = f64_mul(r, x);
    x = f64_mul(x, x);
  }
  return r;
}
// REAL: the root lies in the base field (as in the reference's test and benchmark, fft_test.cc:211-217), so every
// twiddle has a zero imaginary part and its product costs two base-field products instead of three
template <bool REAL>
struct F64x2Ops {
  static constexpr const char* kKey = "f64x2";
  static LF_HD elt_t add(elt_t a, elt_t b) { return f64x2_add(a, b); }
  static LF_HD elt_t sub(elt_t a, elt_t b) { return f64x2_sub(a, b); }
  static LF_HD elt_t mul_tw(elt_t a, elt_t w) { return REAL ? f64x2_mul_real(a, w.lo) : f64x2_mul(a, w); }
  static elt_t hmul(elt_t a, elt_t b) { return f64x2_mul(a, b); }
  static elt_t one() { return elt_t{0xFFFFFFFFull, 0ull}; }
  static elt_t inv(elt_t a) {  // Fp2::invert (fp2.h:112-123): conj(a) / (re^2 + im^2)
    const u64 d = f64_add(f64_mul(a.lo, a.lo), f64_mul(a.hi, a.hi));
    return f64x2_mul_real(elt_t{a.lo, f64_sub(0, a.hi)}, h_f64_pow(d, F64_P - 2));
  }
};

// W[i << wshift] = w_T^i (i < T/2).  Optional inter-pass twiddle w_n^{j*(col)}
// = tw_lo[e & 1023] * tw_hi[e >> 10].
template <class O, int R, int FFT_THREADS>
__device__ __forceinline__ void fp_radix_round(elt_t* s, const elt_t* Wl, u32 wsh, u32 logT, u32 logC, u32 st, u32 tid) {
  constexpr u32 N = 1u << R;
  const u32 T = 1u << logT, C = 1u << logC, m = 1u << st;
  for (u32 e = tid; e < (T >> R) * C; e += FFT_THREADS) {
    const u32 c = e & (C - 1), b = e >> logC;
    const u32 j = b & (m - 1);
    const u32 i0 = ((b >> st) << (st + R)) + j;
    elt_t x[N];
    u32 q[N];
#pragma unroll
    for (u32 a = 0; a < N; ++a) {
      q[a] = lds_slot(i0 + a * m, c, logT, logC);
      x[a] = ld16(&s[q[a]]);
    }
#pragma unroll
    for (u32 t = 0; t < (u32)R; ++t) {
      const u32 half = 1u << t;
#pragma unroll
      for (u32 a = 0; a < N; ++a) {
        if (a & half) continue;
        const u32 jj = j + (a & (half - 1)) * m;
        if (t > 0 || j) {
          if ((a & (half - 1)) || j) x[a + half] = O::mul_tw(x[a + half], ld16(&Wl[(size_t)(jj << (logT - 1 - st - t)) << wsh]));
        }
        const elt_t u = x[a], v = x[a + half];
        x[a] = O::add(u, v);
        x[a + half] = O::sub(u, v);
      }
    }
#pragma unroll
    for (u32 a = 0; a < N; ++a) st16(&s[q[a]], x[a]);
  }
}

// tw_hi == nullptr with tw_lo != nullptr: tw_lo is the FULL inter-pass table [j][column] (one product per element
// instead of two; rows of the grid then vary fastest so that a tile's slice of the table stays in L2 while the
// batch rows stream past it).
// WLDS: the stage twiddles sit in LDS behind the tile (p.wlds; always, for 2^12-element tiles) -- a template parameter so that
// their reads are LDS instructions with 32-bit addresses instead of flat loads through a generic pointer
template <class O, int FFT_THREADS, bool WLDS>
__global__ __launch_bounds__(FFT_THREADS) void fp_fft_tile(TilePlan p, const elt_t* __restrict__ W, u32 wshift,
                                                           const elt_t* __restrict__ tw_lo,
                                                           const elt_t* __restrict__ tw_hi, u32 row_fast) {
  extern __shared__ elt_t s[];
  const u32 T = 1u << p.logT, C = 1u << p.logC, tid = threadIdx.x;
  const u32 bx = row_fast ? blockIdx.y : blockIdx.x, by = row_fast ? blockIdx.x : blockIdx.y;  // (tile, batch row)
  const u32 cbase = bx << p.logC;
  const elt_t* src = p.src + (long long)by * p.src_row + (long long)bx * p.src_tile;
  elt_t* dst = p.dst + (long long)by * p.dst_row + (long long)bx * p.dst_tile;

  for (u32 e = tid; e < T * C; e += FFT_THREADS) {
    u32 k, c;
    if (p.kfast_src) { k = e & (T - 1); c = e >> p.logT; } else { c = e & (C - 1); k = e >> p.logC; }
    elt_t v = elt_zero();
    if (cbase + c < p.nbatch) v = ld16(src + (long long)k * p.sk + (long long)c * p.sc);
    st16(&s[lds_slot(bitrev(k, p.logT), c, p.logT, p.logC)], v);
  }
  // the T/2 stage twiddles w_T^i go behind the tile in LDS: three twiddle reads per radix-4 step then cost an LDS
  // access instead of a vector-memory instruction each
  elt_t* const wl = s + (T << p.logC);  // stage twiddle i at Wl[i << wsh]
  if (WLDS)
    for (u32 i = tid; i < (T >> 1); i += FFT_THREADS) st16(&wl[i], ld16(&W[(size_t)i << wshift]));
  const u32 wsh = WLDS ? 0 : wshift;
  __syncthreads();
  // R stages per LDS round trip on 2^R register-resident points x[a] = s[i0 + a*m]: sub-stage t pairs (a, a + 2^t)
  // with w_T^(jj * T / (2m 2^t)), jj = j + (a mod 2^t) * m.  Same products as radix 2, 1/R of the LDS traffic and
  // barriers, and 2^(R-1) independent carry chains in flight per thread.
  u32 st = 0;
  while (st < p.logT) {
    const u32 rem = p.logT - st;
    const u32 R = (rem == 3 || rem > 4) ? 3 : (rem >= 2 ? 2 : 1);
    if (WLDS) {
      if (R == 3) fp_radix_round<O, 3, FFT_THREADS>(s, wl, wsh, p.logT, p.logC, st, tid);
      else if (R == 2) fp_radix_round<O, 2, FFT_THREADS>(s, wl, wsh, p.logT, p.logC, st, tid);
      else fp_radix_round<O, 1, FFT_THREADS>(s, wl, wsh, p.logT, p.logC, st, tid);
    } else {
      if (R == 3) fp_radix_round<O, 3, FFT_THREADS>(s, W, wsh, p.logT, p.logC, st, tid);
      else if (R == 2) fp_radix_round<O, 2, FFT_THREADS>(s, W, wsh, p.logT, p.logC, st, tid);
      else fp_radix_round<O, 1, FFT_THREADS>(s, W, wsh, p.logT, p.logC, st, tid);
    }
    __syncthreads();
    st += R;
  }
  for (u32 e = tid; e < T * C; e += FFT_THREADS) {
    u32 j, c;
    if (p.kfast_dst) { j = e & (T - 1); c = e >> p.logT; } else { c = e & (C - 1); j = e >> p.logC; }
    if (cbase + c >= p.nbatch) continue;
    elt_t v = ld16(&s[lds_slot(j, c, p.logT, p.logC)]);
    if (tw_lo) {
      const u32 col = cbase + c, ex = j * col;
      if (ex) {
        if (tw_hi) {
          elt_t t = ld16(&tw_lo[ex & 1023]);
          if (ex >> 10) t = O::mul_tw(t, ld16(&tw_hi[ex >> 10]));
          v = O::mul_tw(v, t);
        } else {
          v = O::mul_tw(v, ld16(&tw_lo[(size_t)j * p.nbatch + col]));
        }
      }
    }
    st16(dst + (long long)j * p.dk + (long long)c * p.dc, v);
  }
}

// ------------------------------------------------------------------ K1: the 1024 x 4 tile
// Pass B runs T = 1024 points x C = 4 columns for every n >= 2^13, and at n = 2^20 pass A does too: fp_fft_tile_1024x4 is that
// one tile on 512 threads (8 points each), with the round schedule, lane maps and LDS offsets fixed at compile time.
//   round 0 (stages 0-2): in registers, straight from HBM.  Thread (kb, c) loads points k = kb + 128 a' (a' < 8), which are the
//           radix-8 group b = bitrev7(kb) of bit-reversed positions 8b + a (a' = bitrev3(a)); all 8 loads are issued before
//           the first wait, and the stage twiddles go from HBM to LDS beside them.  Its twiddles (j = 0) are uniform and its
//           w^0 products are left out at compile time.
//   round 1 (stages 3-5, radix 8), round 2 (stages 6-7, radix 4, two groups per thread): LDS -> registers -> LDS.
//   round 3 (stages 8-9, radix 4, two groups per thread): LDS -> registers -> (pass A: x w_n^(j1 k2)) -> HBM.
// Rounds 1-3 multiply by every twiddle, w^0 = Montgomery 1 included (fp_mul(a, 1) = a for a < p): no per-lane branch.
// Three barriers and three LDS round trips per tile instead of the generic kernel's five.
// The rounds are the t4_round* helpers below, shared by the three kernel bodies (fp_fft_tile_1024x4, _persist, _tws_body); what a
// body keeps to itself is its global loads and stores, the inter-pass product and its barriers.
//
// The arithmetic of the 1024 x 4 tiles: O's own, except for Fp128, whose add, sub and twiddle product come from
// fp_tile_arith.h (same values, fewer VALU instructions).  add_lazy / canon: the lazy u side of a butterfly (fp_tile_arith.h),
// for Fp128 only; any other field adds as usual and has nothing to make canonical.
// mul_tw(x, w): the SECOND argument is a twiddle, canonical (< p) as the host builds every table (fp_root_table and the full table
// of fp_fft_two_pass: O::one() and outputs of the host product O::hmul): a stage twiddle out of LDS or W
// (t4_stages) or an entry of the inter-pass table (pass A's store side, pass B's load side).  fpt_mul rests on that: it leaves
// out three carry captures that b3 <= 0xfffff000 makes impossible.  x may be lazy.  Never swap the two.
// mul_tw_sw(x, w): the same product for a wave-uniform w held in SGPRs (fpt_mul_sw); fp_fft_tile_1024x4_tw2 only.
template <class O>
struct T4Ops : O {
  static __device__ __forceinline__ elt_t add_lazy(elt_t a, elt_t b) { return O::add(a, b); }
  static __device__ __forceinline__ elt_t canon(elt_t a) { return a; }
  static __device__ __forceinline__ elt_t mul_tw_sw(elt_t a, elt_t w) { return O::mul_tw(a, w); }
  // the paired forms of fp_fft_tile_1024x4_ilp, in place: two products, two values made canonical, (x, y) <- (x + y lazy, x - y)
  static __device__ __forceinline__ void mul2_tw(elt_t& a, elt_t w, elt_t& b, elt_t v) { a = O::mul_tw(a, w), b = O::mul_tw(b, v); }
  static __device__ __forceinline__ void mul2_tw_sw(elt_t& a, elt_t w, elt_t& b, elt_t v) { mul2_tw(a, w, b, v); }
  static __device__ __forceinline__ void canon2(elt_t&, elt_t&) {}
  static __device__ __forceinline__ void bfly_lazy(elt_t& x, elt_t& y) {
    const elt_t u = x, t = y;
    x = O::add(u, t), y = O::sub(u, t);
  }
  static __device__ __forceinline__ void bfly2_lazy(elt_t& xp, elt_t& yp, elt_t& xq, elt_t& yq) { bfly_lazy(xp, yp), bfly_lazy(xq, yq); }
  // fp_fft_tile_1024x4_lean: two butterflies with full sums on canonical inputs
  static __device__ __forceinline__ void bfly2_full(elt_t& xp, elt_t& yp, elt_t& xq, elt_t& yq) { bfly_lazy(xp, yp), bfly_lazy(xq, yq); }
};
#if defined(__HIP_DEVICE_COMPILE__)
template <>
struct T4Ops<Fp128Ops> : Fp128Ops {
  static __device__ __forceinline__ elt_t add(elt_t a, elt_t b) { return fpt_add(a, b); }
  static __device__ __forceinline__ elt_t add_lazy(elt_t a, elt_t b) { return fpt_add_lazy(a, b); }
  static __device__ __forceinline__ elt_t canon(elt_t a) { return fpt_canon(a); }
  static __device__ __forceinline__ elt_t sub(elt_t a, elt_t b) { return fpt_sub(a, b); }
  static __device__ __forceinline__ elt_t mul_tw(elt_t a, elt_t w) { return fpt_mul(a, w); }
  static __device__ __forceinline__ elt_t mul_tw_sw(elt_t a, elt_t w) { return fpt_mul_sw(a, w); }  // w wave-uniform, in SGPRs
  static __device__ __forceinline__ void mul2_tw(elt_t& a, elt_t w, elt_t& b, elt_t v) { fpt_mul2(a, w, b, v); }
  static __device__ __forceinline__ void mul2_tw_sw(elt_t& a, elt_t w, elt_t& b, elt_t v) { fpt_mul2_sw(a, w, b, v); }  // w, v wave-uniform
  static __device__ __forceinline__ void canon2(elt_t& a, elt_t& b) { fpt_canon2(a, b); }
  static __device__ __forceinline__ void bfly_lazy(elt_t& x, elt_t& y) { fpt_bfly_lazy(x, y); }
  static __device__ __forceinline__ void bfly2_lazy(elt_t& xp, elt_t& yp, elt_t& xq, elt_t& yq) { fpt_bfly2_lazy(xp, yp, xq, yq); }
  static __device__ __forceinline__ void bfly2_full(elt_t& xp, elt_t& yp, elt_t& xq, elt_t& yq) { fpt_bfly2_full(xp, yp, xq, yq); }
};
#endif
// T4Ilp<O>: the field O, its tile arithmetic issued in pairs.  fp_fft_tile_1024x4_tw2<T4Ilp<O>, ..> is the kernel
// fp_fft_tile_1024x4_tw2<O, ..> with the stage helpers t4i_* in place of t4w_stages and t4_stages: one kernel source for both, and
// the instantiation for O itself is untouched by the other's existence.
template <class O>
struct T4Ilp : O {};
template <class O>
struct T4IsIlp : std::false_type {};
template <class O>
struct T4IsIlp<T4Ilp<O>> : std::true_type {};
template <class O>
struct T4Ops<T4Ilp<O>> : T4Ops<O> {};

// LDS layout of the tile, defined here and nowhere else: position p (bit-reversed order), column c at slot (4p + c) ^ (p >> 7),
// the XOR staying inside an aligned 16-slot row.  It is conflict-free for every access of the four rounds (ds_write_b128: 8 x 8
// consecutive lanes on 32 banks, ds_read_b128: 4 x 16 lanes on 64 banks).  Each round's lanes hold positions base + stride a;
// t4_slot gives the slot of the base, and since p >> 7 moves with a only in rounds 2 and 3, the other slots are that one plus an
// immediate offset, with one more XOR of a constant where a reaches bit 7 of the position.
// The stage twiddles w_1024^i (i < 512) sit behind the tile (wl = s + 4096) at slot i ^ ((i >> 4) & 15).
__device__ __forceinline__ u32 t4_slot(u32 p, u32 c, u32 p7) { return ((p << 2) | c) ^ p7; }  // p7 = p >> 7, as the round knows it
__device__ __forceinline__ u32 t4_wslot(u32 i) { return i ^ ((i >> 4) & 15u); }

// R radix-2 stages (from stage ST) on the register group x[a] = position i0 + a 2^ST, j = i0 mod 2^ST; as fp_radix_round.
// ROUND0 (ST = 0, j = 0): twiddles read from HBM at uniform addresses, the w^0 products left out.
// LZ, which sums are canonical.  T4_CANON: all of them (inputs canonical).  T4_LAZY: x[] may come in and go out lazy; u + w v is
// add_lazy, whose v must be canonical: it is wherever v has just been multiplied, which leaves the w^0 butterflies of ROUND0.
// Their v are x[2], x[6] at stage 1 and x[4] at stage 2, so the sums that make them stay full adds on canonical inputs: (2,3),
// (6,7), (4,5) at stage 0 (a round 0's inputs are canonical) and (4,6) at stage 1.  T4_LAZY_OUT: as T4_LAZY, and the outputs are
// canonical: the last stage makes its u canonical and adds in full.
enum : u32 { T4_CANON = 0, T4_LAZY = 1, T4_LAZY_OUT = 2 };
template <class O, u32 ST, u32 R, bool ROUND0, u32 LZ = T4_CANON>
__device__ __forceinline__ void t4_stages(elt_t* x, u32 j, const elt_t* wl, const elt_t* __restrict__ W, u32 wshift) {
#pragma unroll
  for (u32 t = 0; t < R; ++t) {
    const u32 half = 1u << t;
#pragma unroll
    for (u32 a = 0; a < (1u << R); ++a) {
      if (a & half) continue;
      const u32 jj = j + (a & (half - 1)) * (1u << ST), sh = 9 - ST - t;
      if (!ROUND0) x[a + half] = T4Ops<O>::mul_tw(x[a + half], ld16(&wl[t4_wslot(jj << sh)]));
      else if (a & (half - 1)) x[a + half] = T4Ops<O>::mul_tw(x[a + half], ld16(&W[(size_t)(jj << sh) << wshift]));
      const bool last = LZ == T4_LAZY_OUT && t == R - 1;
      const bool full = LZ == T4_CANON || last || (ROUND0 && ((t == 0 && a != 0) || (t == 1 && a == 4)));
      const elt_t u = last ? T4Ops<O>::canon(x[a]) : x[a], v = x[a + half];
      x[a] = full ? T4Ops<O>::add(u, v) : T4Ops<O>::add_lazy(u, v);
      x[a + half] = T4Ops<O>::sub(u, v);
    }
  }
}

// Round 0 of thread (kb, c), whose y[a'] is point kb + 128 a' of column c: stages 0-2 on x[a] = y[bitrev3(a)], then positions
// 8b + a to LDS.  8b >> 7 = b >> 4 reaches bit 2 of the slot, so odd a have a base of their own.
template <class O, u32 LZ>
__device__ __forceinline__ void t4_round0(elt_t* s, const elt_t* y, u32 kb, u32 c, const elt_t* wl, const elt_t* __restrict__ W, u32 wshift) {
  elt_t x[8];
#pragma unroll
  for (u32 a = 0; a < 8; ++a) x[a] = y[((a & 1) << 2) | (a & 2) | (a >> 2)];
  t4_stages<O, 0, 3, true, LZ>(x, 0, wl, W, wshift);
  const u32 b = __brev(kb) >> 25, s0 = t4_slot(8 * b, c, b >> 4), s1 = t4_slot(8 * b + 1, c, b >> 4);
#pragma unroll
  for (u32 a = 0; a < 8; a += 2) {
    st16(&s[s0 + 4 * a], x[a]);
    st16(&s[s1 + 4 * a], x[a + 1]);
  }
}
// Round 1: group (c, j < 8, h < 16) = positions 64h + j + 8a; (p >> 7) = h >> 1 for all eight.
template <class O, u32 LZ>
__device__ __forceinline__ void t4_round1(elt_t* s, u32 tid, const elt_t* wl, const elt_t* __restrict__ W, u32 wshift) {
  const u32 c = tid & 3, j = (tid >> 2) & 7, h = tid >> 5;
  const u32 s0 = t4_slot(64 * h + j, c, h >> 1);
  elt_t x[8];
#pragma unroll
  for (u32 a = 0; a < 8; ++a) x[a] = ld16(&s[s0 + 32 * a]);
  t4_stages<O, 3, 3, false, LZ>(x, j, wl, W, wshift);
#pragma unroll
  for (u32 a = 0; a < 8; ++a) st16(&s[s0 + 32 * a], x[a]);
}
// Round 2, one group e = tid + 512 g: (c, j < 64, h < 4) = positions 256h + j + 64a; (p >> 7) = 2h + (a >> 1).  In two halves,
// because fp_fft_tile_1024x4 issues its table loads between the LDS loads and the stages; the first returns the group's base
// slot for the second.
__device__ __forceinline__ u32 t4_round2_load(elt_t* x, const elt_t* s, u32 e) {
  const u32 c = e & 3, h = e >> 8, j = (e >> 2) & 63;
  const u32 s0 = t4_slot(256 * h + j, c, 2 * h);
#pragma unroll
  for (u32 a = 0; a < 4; ++a) x[a] = ld16(&s[(s0 ^ (a >> 1)) + 256 * a]);
  return s0;
}
template <class O, u32 LZ>
__device__ __forceinline__ void t4_round2_finish(elt_t* s, elt_t* x, u32 e, u32 s0, const elt_t* wl, const elt_t* __restrict__ W, u32 wshift) {
  t4_stages<O, 6, 2, false, LZ>(x, (e >> 2) & 63, wl, W, wshift);
#pragma unroll
  for (u32 a = 0; a < 4; ++a) st16(&s[(s0 ^ (a >> 1)) + 256 * a], x[a]);
}
template <class O, u32 LZ>
__device__ __forceinline__ void t4_round2(elt_t* s, u32 e, const elt_t* wl, const elt_t* __restrict__ W, u32 wshift) {
  elt_t x[4];
  const u32 s0 = t4_round2_load(x, s, e);
  t4_round2_finish<O, LZ>(s, x, e, s0, wl, W, wshift);
}
// Round 3's LDS loads of one group e = tid + 512 g: (c, j < 256) = (e & 3, e >> 2), positions (= output points) j + 256a;
// (p >> 7) = (j >> 7) + 2a.  Lanes walk c, then j.  The stages t4_stages<O, 8, 2, false, LZ>(x, e >> 2, ..) and the stores are the caller's.
__device__ __forceinline__ void t4_round3_load(elt_t* x, const elt_t* s, u32 e) {
  const u32 c = e & 3, j = e >> 2;
  const u32 s0 = t4_slot(j, c, j >> 7);
#pragma unroll
  for (u32 a = 0; a < 4; ++a) x[a] = ld16(&s[(s0 ^ (2 * a)) + 1024 * a]);
}

// XCD-aware tile order of pass A's 1-D grids: workgroup w = 8i + x (x: the blocks that share an XCD, blocks being dealt round-robin
// over the 8 XCDs) takes column block bx = (ncb/8) x + i mod (ncb/8) and part i / (ncb/8) of the rows.  The workgroups of one XCD
// then read adjacent 64-byte segments of the same rows at about the same time, and its L2 holds only their 1/8 of the twiddle table.
__device__ __forceinline__ void t4_xcd_order(u32 ncb, u32 w, u32& bx, u32& part) {
  if ((ncb & 7) == 0) {
    const u32 per = ncb >> 3, i = w >> 3;
    bx = (w & 7) * per + i % per;
    part = i / per;
  } else {
    bx = w % ncb;
    part = w / ncb;
  }
}
// Pass A's inter-pass twiddles of a thread's eight round-3 outputs j1 = j + 256a of column block cbase / 4, from the full table:
// w_n^(j1 k2) = tw[j1 * nbatch + k2]
__device__ __forceinline__ void t4a_tw_load(elt_t (*t)[4], const elt_t* __restrict__ tw, u32 nbatch, u32 cbase, u32 tid) {
#pragma unroll
  for (u32 g = 0; g < 2; ++g) {
    const u32 e = tid + 512 * g;
#pragma unroll
    for (u32 a = 0; a < 4; ++a) t[g][a] = ld16(&tw[(size_t)((e >> 2) + 256 * a) * nbatch + cbase + (e & 3)]);
  }
}

// KFAST_SRC: pass B (points contiguous, columns n2 apart); otherwise pass A (columns contiguous).  The store side is columns
// contiguous in both passes (kfast_dst = 0).  TW: pass A's inter-pass product with the full [j][column] table.
// Needs p.logT = 10, p.logC = 2, p.wlds, p.nbatch a multiple of 4 (no partial tiles).
template <class O, bool KFAST_SRC, bool TW>
__global__ __launch_bounds__(512, 4) void fp_fft_tile_1024x4(TilePlan p, const elt_t* __restrict__ W, u32 wshift,
                                                             const elt_t* __restrict__ tw, u32 row_fast) {
  extern __shared__ elt_t s[];
  elt_t* const wl = s + 4096;
  const u32 tid = threadIdx.x;
  const u32 bx = row_fast ? blockIdx.y : blockIdx.x, by = row_fast ? blockIdx.x : blockIdx.y;  // (tile, batch row)
  {  // round 0.  Pass B: a wave reads 64 consecutive points of one column; pass A: 16 rows of 4 consecutive columns.
    const u32 c = KFAST_SRC ? tid >> 7 : tid & 3, kb = KFAST_SRC ? tid & 127 : tid >> 2;
    const elt_t* src = p.src + (long long)by * p.src_row + (long long)bx * p.src_tile + (long long)kb * p.sk + (long long)c * p.sc;
    elt_t y[8];
#pragma unroll
    for (u32 a = 0; a < 8; ++a) y[a] = ld16(src + (long long)(128 * a) * p.sk);
    const elt_t wv = ld16(&W[(size_t)tid << wshift]);
    __builtin_amdgcn_sched_barrier(0);  // all nine loads in flight before the first wait (the scheduler would sink them)
    t4_round0<O, T4_CANON>(s, y, kb, c, wl, W, wshift);
    st16(&wl[t4_wslot(tid)], wv);
  }
  __syncthreads();
  t4_round1<O, T4_CANON>(s, tid, wl, W, wshift);
  __syncthreads();
  elt_t t[2][4];  // pass A: the inter-pass twiddles of round 3's outputs
  {  // round 2, with pass A's eight table loads in flight during rounds 2 and 3
    elt_t x[2][4];
    u32 s0[2];
#pragma unroll
    for (u32 g = 0; g < 2; ++g) s0[g] = t4_round2_load(x[g], s, tid + 512 * g);
    if (TW) {
      t4a_tw_load(t, tw, p.nbatch, bx << 2, tid);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (u32 g = 0; g < 2; ++g) t4_round2_finish<O, T4_CANON>(s, x[g], tid + 512 * g, s0[g], wl, W, wshift);
  }
  __syncthreads();
  {  // round 3
    elt_t* dst = p.dst + (long long)by * p.dst_row + (long long)bx * p.dst_tile;
#pragma unroll
    for (u32 g = 0; g < 2; ++g) {
      const u32 e = tid + 512 * g, c = e & 3, j = e >> 2;
      elt_t x[4];
      t4_round3_load(x, s, e);
      t4_stages<O, 8, 2, false>(x, j, wl, W, wshift);
#pragma unroll
      for (u32 a = 0; a < 4; ++a) {
        if (TW) x[a] = T4Ops<O>::mul_tw(x[a], t[g][a]);
        st16(dst + (long long)(j + 256 * a) * p.dk + (long long)c * p.dc, x[a]);
      }
    }
  }
}

// Pass A's round-0 loads of tile (row by, column block bx): thread (kb, c) = (tid >> 2, tid & 3) reads points kb + 128 a'.
// Offsets inside the row in 32 bits (the host keeps 1024 sk + 4 sc below 2^32).
__device__ __forceinline__ void t4a_load(elt_t* y, const TilePlan& p, u32 by, u32 bx, u32 tid) {
  const elt_t* src = p.src + (long long)by * p.src_row + (long long)bx * p.src_tile;
  const u32 sk = (u32)p.sk, off = (tid >> 2) * sk + (tid & 3) * (u32)p.sc;
#pragma unroll
  for (u32 a = 0; a < 8; ++a) y[a] = ld16(src + (off + 128 * a * sk));
}

// Pass A (columns contiguous, inter-pass product) in the XCD-aware tile order (t4_xcd_order), optionally as a tile loop: the same
// rounds as fp_fft_tile_1024x4.  With parts < rows each workgroup keeps one column block bx and walks down a range of batch rows,
// so what depends on bx alone is loaded once (with parts = rows, the default, every workgroup takes one tile):
//   - the eight inter-pass twiddles w_n^(j1 k2) of each thread stay in registers (t) for every tile;
//   - the stage twiddles go to LDS once.
// Grid: ncb * parts workgroups (ncb = p.nbatch / 4 column blocks); part q covers rows [q rows / parts, (q + 1) rows / parts).
template <class O>
__global__ __launch_bounds__(512, 4) void fp_fft_tile_1024x4_persist(TilePlan p, const elt_t* __restrict__ W, u32 wshift,
                                                                     const elt_t* __restrict__ tw, u32 rows, u32 parts) {
  extern __shared__ elt_t s[];
  elt_t* const wl = s + 4096;
  const u32 tid = threadIdx.x;
  u32 bx, part;
  t4_xcd_order(p.nbatch >> 2, blockIdx.x, bx, part);
  const u32 r0 = (u32)((u64)part * rows / parts), r1 = (u32)((u64)(part + 1) * rows / parts);
  elt_t y[8], t[2][4];
  t4a_tw_load(t, tw, p.nbatch, bx << 2, tid);
  st16(&wl[t4_wslot(tid)], ld16(&W[(size_t)tid << wshift]));  // read after the first tile's first barrier
  for (u32 by = r0; by < r1; ++by) {
    // every per-lane index below is recomputed per tile from lt: hoisted out of the loop, the addresses would hold more VGPRs
    // than the 128 of four waves per SIMD
    u32 lt = tid;
    asm volatile("" : "+v"(lt));
    t4a_load(y, p, by, bx, lt);
    __builtin_amdgcn_sched_barrier(0);  // all eight in flight before the first wait, as in fp_fft_tile_1024x4
    t4_round0<O, T4_CANON>(s, y, lt >> 2, lt & 3, wl, W, wshift);
    __syncthreads();
    t4_round1<O, T4_CANON>(s, lt, wl, W, wshift);
    __syncthreads();
#pragma unroll
    for (u32 g = 0; g < 2; ++g) t4_round2<O, T4_CANON>(s, lt + 512 * g, wl, W, wshift);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);  // keeps round 2's and round 3's instructions apart: interleaved, they spill
    {  // round 3: both groups out of LDS first; after the barrier the tile's LDS belongs to the next tile's round 0 (one barrier
       // more per tile than fp_fft_tile_1024x4; this order needs fewer VGPRs than a barrier at the end of the loop)
      elt_t x[2][4];
#pragma unroll
      for (u32 g = 0; g < 2; ++g) t4_round3_load(x[g], s, lt + 512 * g);
      __syncthreads();
      elt_t* dst = p.dst + (long long)by * p.dst_row + (long long)bx * p.dst_tile;
      const u32 dk = (u32)p.dk, dc = (u32)p.dc;
#pragma unroll
      for (u32 g = 0; g < 2; ++g) {
        const u32 e = lt + 512 * g, c = e & 3, j = e >> 2;
        t4_stages<O, 8, 2, false>(x[g], j, wl, W, wshift);
#pragma unroll
        for (u32 a = 0; a < 4; ++a) st16(dst + ((j + 256 * a) * dk + c * dc), T4Ops<O>::mul_tw(x[g][a], t[g][a]));
      }
    }
  }
}

// The 1024 x 4 tile with the inter-pass product on pass B's load side (n = 2^20, the default): same rounds as fp_fft_tile_1024x4,
// every offset inside a tile in 32 bits (the host keeps 1024 sk + 4 sc and 1024 dk + 4 dc below 2^32).
//   pass A (KFAST_SRC = false): no table and no product.  1-D grid of ncb * rows workgroups in the XCD-aware tile order
//           (t4_xcd_order, parts = rows): the workgroups of one XCD read adjacent 64-byte segments of the same rows.
//   pass B (KFAST_SRC = true): what pass A wrote is laid out [j1][k2] like the full table tw[j1 * 1024 + k2], so thread (kb, c)
//           loads w_n^(j1 k2) at the offset of its point (j1 = 4 bx + c, k2 = kb + 128 a'), coalesced, all 17 loads in flight
//           before the first wait, and multiplies before round 0.  Row j1 = 0 and column k2 = 0 hold Montgomery 1: no branch.
//           Grid (tile, row), or (row, tile) with row_fast.
// LAZY (the default, fp_fft_tile_1024x4_tws; LFGPU_FP_LAZY=0 launches fp_fft_tile_1024x4_tws_canon, the same body with LAZY = false):
// the butterflies keep their u side lazy (t4_stages, fp_tile_arith.h), which takes 3 of the 21 instructions off 36 of a thread's 40
// butterflies in pass A and off 32 in pass B.  What the tile keeps in LDS may then be any 128-bit representative, and so may what
// pass A stores; pass B's last stage makes its outputs canonical, so the transform's result is the same bytes.  Pass A's destination
// in this plan is fp_fft_two_pass's scratch buffer and nothing else, and the only reader of that buffer is the pass B launched right
// behind it, tiles or rows fastest (LFGPU_FP_TWSIDE=2), which multiplies every point by its inter-pass twiddle before anything
// else: a product takes a lazy operand and gives a canonical one.  The inner 2^20-point transforms of n = 2^21 .. 2^23 are the same
// two launches through the same scratch buffer; their pass A reads what fp_fft_tile stored (canonical) and their pass B stores
// canonical values with a stride.  Every other kernel of this file keeps canonical arithmetic.
template <class O, bool KFAST_SRC, bool LAZY>
__device__ __forceinline__ void fp_fft_tile_1024x4_tws_body(const TilePlan& p, const elt_t* __restrict__ W, u32 wshift,
                                                            const elt_t* __restrict__ tw, u32 row_fast) {
  constexpr u32 LZ = LAZY ? T4_LAZY : T4_CANON, LZ_OUT = !LAZY ? T4_CANON : KFAST_SRC ? T4_LAZY_OUT : T4_LAZY;
  extern __shared__ elt_t s[];
  elt_t* const wl = s + 4096;
  const u32 tid = threadIdx.x;
  u32 bx, by;  // (tile, batch row)
  if (KFAST_SRC) {
    bx = row_fast ? blockIdx.y : blockIdx.x;
    by = row_fast ? blockIdx.x : blockIdx.y;
  } else {
    t4_xcd_order(p.nbatch >> 2, blockIdx.x, bx, by);
  }
  {  // round 0
    const u32 c = KFAST_SRC ? tid >> 7 : tid & 3, kb = KFAST_SRC ? tid & 127 : tid >> 2;
    const elt_t* src = p.src + (long long)by * p.src_row + (long long)bx * p.src_tile;
    const u32 sk = (u32)p.sk, off = kb * sk + c * (u32)p.sc;
    elt_t y[8], t[8];
#pragma unroll
    for (u32 a = 0; a < 8; ++a) y[a] = ld16(src + (off + 128 * a * sk));
    if (KFAST_SRC) {
      const elt_t* twt = tw + ((size_t)bx << 12);
      const u32 toff = (c << 10) + kb;
#pragma unroll
      for (u32 a = 0; a < 8; ++a) t[a] = ld16(twt + (toff + 128 * a));
    }
    const elt_t wv = ld16(&W[(size_t)tid << wshift]);
    __builtin_amdgcn_sched_barrier(0);  // every load in flight before the first wait, as in fp_fft_tile_1024x4
    if (KFAST_SRC) {
#pragma unroll
      for (u32 a = 0; a < 8; ++a) y[a] = T4Ops<O>::mul_tw(y[a], t[a]);
    }
    t4_round0<O, LZ>(s, y, kb, c, wl, W, wshift);
    st16(&wl[t4_wslot(tid)], wv);
  }
  __syncthreads();
  t4_round1<O, LZ>(s, tid, wl, W, wshift);
  __syncthreads();
#pragma unroll
  for (u32 g = 0; g < 2; ++g) t4_round2<O, LZ>(s, tid + 512 * g, wl, W, wshift);
  __syncthreads();
  {  // round 3
    elt_t* dst = p.dst + (long long)by * p.dst_row + (long long)bx * p.dst_tile;
    const u32 dk = (u32)p.dk, dc = (u32)p.dc;
#pragma unroll
    for (u32 g = 0; g < 2; ++g) {
      const u32 e = tid + 512 * g, c = e & 3, j = e >> 2;
      elt_t x[4];
      t4_round3_load(x, s, e);
      t4_stages<O, 8, 2, false, LZ_OUT>(x, j, wl, W, wshift);
#pragma unroll
      for (u32 a = 0; a < 4; ++a) st16(dst + ((j + 256 * a) * dk + c * dc), x[a]);
    }
  }
}

template <class O, bool KFAST_SRC>
__global__ __launch_bounds__(512, 4) void fp_fft_tile_1024x4_tws(TilePlan p, const elt_t* __restrict__ W, u32 wshift,
                                                                 const elt_t* __restrict__ tw, u32 row_fast) {
  fp_fft_tile_1024x4_tws_body<O, KFAST_SRC, true>(p, W, wshift, tw, row_fast);
}
template <class O, bool KFAST_SRC>
__global__ __launch_bounds__(512, 4) void fp_fft_tile_1024x4_tws_canon(TilePlan p, const elt_t* __restrict__ W, u32 wshift,
                                                                       const elt_t* __restrict__ tw, u32 row_fast) {
  fp_fft_tile_1024x4_tws_body<O, KFAST_SRC, false>(p, W, wshift, tw, row_fast);
}

// ------------------------------------------------------------------ K1: the 1024 x 4 pair with a wave-uniform round 1
// fp_fft_tile_1024x4_tw2 is fp_fft_tile_1024x4_tws (LAZY) with another lane map in round 1 and, to carry it, another LDS layout;
// loads, stores, the inter-pass product, the lazy rules of rounds 0, 2 and 3 and the bytes that come out are the same.  Round 0's
// three uniform twiddles (w^128, w^256, w^384) are scalar operands of its products like round 1's, not moved into VGPRs.  It has
// round helpers and a slot function of its own (t4w_*): t4_slot and the t4_round* above belong to the kernels above.
// Its instantiation for T4Ilp<Fp128Ops> (LFGPU_FP_LEAN=0 launches it, and LFGPU_FP_ILP=0 the one for Fp128Ops; the default is
// fp_fft_tile_1024x4_lean further down, which computes the same) is the same kernel with the stage helpers
// t4i_*, which issue a stage's products, canons and butterflies two at a time (fp_tile_arith.h), carry links filled with the
// other operation's instructions instead of s_nop.  Same values and VALU counts; DESIGN 4.1, profiles/k1_ilp/.
//
// Round 1.  A wave takes one j: j = tid >> 6 (made scalar), lanes = (c, h) = (lane & 3, lane >> 2), positions 64h + j + 8a.  The
// round has 56 twiddles per workgroup, 7 per j: w_1024^(64 j) for stage 3, ^(32 (j + 8k)), k < 2, for stage 4, ^(16 (j + 8k)),
// k < 4, for stage 5 (t4_stages' jj << sh).  The wave fetches its seven by scalar loads from W, in flight beside the tile's loads,
// and they are the scalar operand of the products (T4Ops::mul_tw_sw): no LDS read and no slot arithmetic for them.  The j = 0
// wave takes a uniform branch to a round without its seven products by w^0 (all four of stage 3, k = 0 of stages 4 and 5), five
// products instead of twelve.  Lazy rule of that wave: a butterfly's v has to be canonical (fpt_add_lazy, fpt_sub), and a v that
// is not multiplied is not.  Round 0's rule (full adds on canonical inputs make those v) does not carry over, because this round's
// inputs come lazy out of round 0: every one of the seven v is either such an input (x[1], x[3], x[5], x[7] at stage 3) or a sum
// whose u is one (x[2], x[6] at stage 4; x[4] at stage 5), and a full add wants u canonical as well.  So each skipped product
// becomes T4Ops::canon(v), 8 instructions for 50; the sums stay lazy.
//
// LDS layout: position p, column c at slot (4p + c) ^ L(p), L(p) = (p >> 7) ^ ((p >> 4) & 12): a GF(2)-linear map of p6..p9 into
// the low four slot bits (p6 -> 4, p7 -> 9, p8 -> 2, p9 -> 4), inside an aligned 16-slot row like (4p + c) ^ (p >> 7), under
// which the (c, h) lanes above would meet 4-way bank conflicts.  With ds_read_b128 served 16 lanes at a time on 64 banks (slots
// mod 16 distinct) and ds_write_b128 8 lanes at a time on 32 banks (slots mod 8 distinct), a lane group is free of conflicts when
//   round-0 write, pass A (lanes c, then p9, ..): L(p9) has bit 2;      pass B (lanes p9, p8, p7, ..): L(p7), L(p8), L(p9) are
//   independent in bits 0-2;      round-1 read (lanes c, p6, p7): L(p6), L(p7) independent in bits 2-3;      round-1 write (c, p6):
//   L(p6) has bit 2;      rounds 2 and 3 (lanes c, p0, p1): always.
// tests/test_fp128_tile_r1wave_layout.py is the model.  Offsets: L moves with the register index a only where a reaches p6..p9.
// Round 0 (positions 8b + a): a & 3 lands in slot bits 2-3, which L also writes, so four bases s0 ^ 4 (a & 3), + 16 for a >= 4.
// Round 1: one base, + 32 a.  Round 2 (a = p6, p7): (s0 ^ L(64 a)) + 256 a.  Round 3 (a = p8, p9): (s0 ^ 2a) + 1024 a.
__device__ __forceinline__ u32 t4w_swz(u32 p) { return (p >> 7) ^ ((p >> 4) & 12u); }  // L(p), p < 1024
__device__ __forceinline__ u32 t4w_slot(u32 p, u32 c) { return ((p << 2) | c) ^ t4w_swz(p); }

// Index into the stage-twiddle table w_1024^i of a radix-8 round's twiddle m < 7 at j, the round starting at stage ST:
// m = 2^t - 1 + k is stage ST + t's (a mod 2^t) = k, as t4_stages' jj << sh
template <u32 ST>
__device__ __forceinline__ u32 t4w_tw_index(u32 j, u32 m) {
  const u32 t = m < 1 ? 0 : m < 3 ? 1 : 2, k = m + 1 - (1u << t);
  return (j + (k << ST)) << (9 - ST - t);
}
// Three stages on the register group x[a] with the wave's seven twiddles w[m] (t4w_tw_index) in SGPRs, all sums lazy but for
// T4W_R0.  T4W_R1: every product.  T4W_R0 and T4W_R1_J0 (j = 0) leave out the products by w^0 (k = 0; w[0], w[1], w[3] are not
// read): T4W_R0 with t4_stages' ROUND0 rule, full adds where a sum becomes the v of such a butterfly; T4W_R1_J0 makes each such v
// canonical (see above).
enum : u32 { T4W_R0 = 0, T4W_R1 = 1, T4W_R1_J0 = 2 };
template <class O, u32 MODE>
__device__ __forceinline__ void t4w_stages(elt_t* x, const elt_t* w) {
#pragma unroll
  for (u32 t = 0; t < 3; ++t) {
    const u32 half = 1u << t;
#pragma unroll
    for (u32 a = 0; a < 8; ++a) {
      if (a & half) continue;
      const u32 k = a & (half - 1);
      const bool skip = MODE != T4W_R1 && k == 0, full = MODE == T4W_R0 && ((t == 0 && a != 0) || (t == 1 && a == 4));
      const elt_t u = x[a], v = !skip ? T4Ops<O>::mul_tw_sw(x[a + half], w[half - 1 + k]) : MODE == T4W_R1_J0 ? T4Ops<O>::canon(x[a + half]) : x[a + half];
      x[a] = full ? T4Ops<O>::add(u, v) : T4Ops<O>::add_lazy(u, v);
      x[a + half] = T4Ops<O>::sub(u, v);
    }
  }
}
// The same three stages for fp_fft_tile_1024x4_ilp: what a stage has of products, of canons and of lazy butterflies is done two
// at a time by the paired routines of fp_tile_arith.h (T4Ops::mul2_tw_sw, canon2, bfly2_lazy), products first, and an odd one
// left over by the single form; round 0's four butterflies with full adds stay on add / sub.  Same values: only the order in
// which independent operations are issued differs.  t4i_plan sorts stage t's four butterflies (named by the index a of u) into
// those lists with t4w_stages' own conditions.
struct T4iStage {
  u32 np, prod[4], nc, can[4], nl, lazy[4], nf, full[4];
};
template <u32 MODE>
constexpr T4iStage t4i_plan(u32 t) {
  T4iStage s{};
  const u32 half = 1u << t;
  for (u32 a = 0; a < 8; ++a) {
    if (a & half) continue;
    const bool skip = MODE != T4W_R1 && (a & (half - 1)) == 0, full = MODE == T4W_R0 && ((t == 0 && a != 0) || (t == 1 && a == 4));
    if (!skip) s.prod[s.np++] = a;
    else if (MODE == T4W_R1_J0) s.can[s.nc++] = a;
    if (full) s.full[s.nf++] = a;
    else s.lazy[s.nl++] = a;
  }
  return s;
}
template <class O, u32 MODE, u32 T>
__device__ __forceinline__ void t4i_stage(elt_t* x, const elt_t* w) {
  constexpr T4iStage S = t4i_plan<MODE>(T);
  constexpr u32 half = 1u << T, first = half - 1;  // stage T's twiddles are w[first + k], k = a mod half
#pragma unroll
  for (u32 i = 0; i + 1 < S.np; i += 2) {
    const u32 a = S.prod[i], b = S.prod[i + 1];
    T4Ops<O>::mul2_tw_sw(x[a + half], w[first + (a & first)], x[b + half], w[first + (b & first)]);
  }
  if constexpr (S.np & 1) x[S.prod[S.np - 1] + half] = T4Ops<O>::mul_tw_sw(x[S.prod[S.np - 1] + half], w[first + (S.prod[S.np - 1] & first)]);
#pragma unroll
  for (u32 i = 0; i + 1 < S.nc; i += 2) T4Ops<O>::canon2(x[S.can[i] + half], x[S.can[i + 1] + half]);
  if constexpr (S.nc & 1) x[S.can[S.nc - 1] + half] = T4Ops<O>::canon(x[S.can[S.nc - 1] + half]);
#pragma unroll
  for (u32 i = 0; i < S.nf; ++i) {
    const u32 a = S.full[i];
    const elt_t u = x[a], v = x[a + half];
    x[a] = T4Ops<O>::add(u, v);
    x[a + half] = T4Ops<O>::sub(u, v);
  }
#pragma unroll
  for (u32 i = 0; i + 1 < S.nl; i += 2) T4Ops<O>::bfly2_lazy(x[S.lazy[i]], x[S.lazy[i] + half], x[S.lazy[i + 1]], x[S.lazy[i + 1] + half]);
  if constexpr (S.nl & 1) T4Ops<O>::bfly_lazy(x[S.lazy[S.nl - 1]], x[S.lazy[S.nl - 1] + half]);
}
template <class O, u32 MODE>
__device__ __forceinline__ void t4i_stages(elt_t* x, const elt_t* w) {
  t4i_stage<O, MODE, 0>(x, w);
  t4i_stage<O, MODE, 1>(x, w);
  t4i_stage<O, MODE, 2>(x, w);
}
// Rounds 2 and 3 (ST = 6, 8), as t4_stages<O, ST, 2, false, LZ> with LZ = T4_LAZY or T4_LAZY_OUT: a radix-4 stage is one pair
template <class O, u32 ST, u32 LZ>
__device__ __forceinline__ void t4i_stages4(elt_t* x, u32 j, const elt_t* wl) {
#pragma unroll
  for (u32 t = 0; t < 2; ++t) {
    const u32 half = 1u << t, a = 0, b = 2 >> t, sh = 9 - ST - t;
    T4Ops<O>::mul2_tw(x[a + half], ld16(&wl[t4_wslot(j << sh)]), x[b + half], ld16(&wl[t4_wslot((j + (b & (half - 1)) * (1u << ST)) << sh)]));
    if (LZ == T4_LAZY_OUT && t == 1) {
      T4Ops<O>::canon2(x[a], x[b]);
#pragma unroll
      for (u32 i = 0; i < 2; ++i) {
        const elt_t u = x[i], v = x[i + half];
        x[i] = T4Ops<O>::add(u, v);
        x[i + half] = T4Ops<O>::sub(u, v);
      }
    } else {
      T4Ops<O>::bfly2_lazy(x[a], x[a + half], x[b], x[b + half]);
    }
  }
}
// The round helpers below serve both pairs: T4IsIlp<O> chooses the stage helper and nothing else.
// Round 0, as t4_round0, with its twiddles w (t4w_tw_index<0>(0, m)) in SGPRs
template <class O>
__device__ __forceinline__ void t4w_round0(elt_t* s, const elt_t* y, u32 kb, u32 c, const elt_t* w) {
  elt_t x[8];
#pragma unroll
  for (u32 a = 0; a < 8; ++a) x[a] = y[((a & 1) << 2) | (a & 2) | (a >> 2)];
  if constexpr (T4IsIlp<O>::value) t4i_stages<O, T4W_R0>(x, w);
  else t4w_stages<O, T4W_R0>(x, w);
  const u32 s0 = t4w_slot((__brev(kb) >> 25) << 3, c);
#pragma unroll
  for (u32 a = 0; a < 8; ++a) st16(&s[(s0 ^ (4 * (a & 3))) + 16 * (a >> 2)], x[a]);
}
// Round 1 of the wave with twiddle index j (uniform): group (c, h < 16) = positions 64h + j + 8a
template <class O, u32 MODE>
__device__ __forceinline__ void t4w_round1_wave(elt_t* s, u32 s0, const elt_t* w) {
  elt_t x[8];
#pragma unroll
  for (u32 a = 0; a < 8; ++a) x[a] = ld16(&s[s0 + 32 * a]);
  if constexpr (T4IsIlp<O>::value) t4i_stages<O, MODE>(x, w);
  else t4w_stages<O, MODE>(x, w);
#pragma unroll
  for (u32 a = 0; a < 8; ++a) st16(&s[s0 + 32 * a], x[a]);
}
// Each path loads and stores for itself: with the eight values joined in registers behind the branch the kernel takes 16 VGPRs
// more.  The two asm comments differ, so the compiler cannot merge the paths' loads and stores again.
template <class O>
__device__ __forceinline__ void t4w_round1(elt_t* s, u32 tid, u32 j, const elt_t* w) {
  const u32 c = tid & 3, h = (tid >> 2) & 15;
  const u32 s0 = t4w_slot(64 * h + j, c);
  if (j == 0) {
    asm volatile("; round 1, j = 0");
    t4w_round1_wave<O, T4W_R1_J0>(s, s0, w);
    asm volatile("; round 1, j = 0: stored");
  } else {
    asm volatile("; round 1, j > 0");
    t4w_round1_wave<O, T4W_R1>(s, s0, w);
    asm volatile("; round 1, j > 0: stored");
  }
}
// Round 2, one group e = tid + 512 g, as t4_round2: positions 256h + j + 64a
template <class O>
__device__ __forceinline__ void t4w_round2(elt_t* s, u32 e, const elt_t* wl, const elt_t* __restrict__ W, u32 wshift) {
  const u32 c = e & 3, h = e >> 8, j = (e >> 2) & 63;
  const u32 s0 = t4w_slot(256 * h + j, c);
  elt_t x[4];
#pragma unroll
  for (u32 a = 0; a < 4; ++a) x[a] = ld16(&s[(s0 ^ t4w_swz(64 * a)) + 256 * a]);
  if constexpr (T4IsIlp<O>::value) t4i_stages4<O, 6, T4_LAZY>(x, j, wl);
  else t4_stages<O, 6, 2, false, T4_LAZY>(x, j, wl, W, wshift);
#pragma unroll
  for (u32 a = 0; a < 4; ++a) st16(&s[(s0 ^ t4w_swz(64 * a)) + 256 * a], x[a]);
}
// Round 3's LDS loads of one group e = tid + 512 g, as t4_round3_load: positions j + 256a
__device__ __forceinline__ void t4w_round3_load(elt_t* x, const elt_t* s, u32 e) {
  const u32 s0 = t4w_slot(e >> 2, e & 3);
#pragma unroll
  for (u32 a = 0; a < 4; ++a) x[a] = ld16(&s[(s0 ^ (2 * a)) + 1024 * a]);
}

template <class O, bool KFAST_SRC>
__global__ __launch_bounds__(512, 4) void fp_fft_tile_1024x4_tw2(TilePlan p, const elt_t* __restrict__ W, u32 wshift,
                                                                 const elt_t* __restrict__ tw, u32 row_fast) {
  extern __shared__ elt_t s[];
  elt_t* const wl = s + 4096;
  const u32 tid = threadIdx.x, j1 = __builtin_amdgcn_readfirstlane(tid >> 6);
  u32 bx, by;  // (tile, batch row)
  if (KFAST_SRC) {
    bx = row_fast ? blockIdx.y : blockIdx.x;
    by = row_fast ? blockIdx.x : blockIdx.y;
  } else {
    t4_xcd_order(p.nbatch >> 2, blockIdx.x, bx, by);
  }
  elt_t w0[7] = {}, w1[7];  // the stage twiddles of rounds 0 and 1
  {  // round 0
    const u32 c = KFAST_SRC ? tid >> 7 : tid & 3, kb = KFAST_SRC ? tid & 127 : tid >> 2;
    const elt_t* src = p.src + (long long)by * p.src_row + (long long)bx * p.src_tile;
    const u32 sk = (u32)p.sk, off = kb * sk + c * (u32)p.sc;
    elt_t y[8], t[8];
#pragma unroll
    for (u32 a = 0; a < 8; ++a) y[a] = ld16(src + (off + 128 * a * sk));
    if (KFAST_SRC) {
      const elt_t* twt = tw + ((size_t)bx << 12);
      const u32 toff = (c << 10) + kb;
#pragma unroll
      for (u32 a = 0; a < 8; ++a) t[a] = ld16(twt + (toff + 128 * a));
    }
    const elt_t wv = ld16(&W[(size_t)tid << wshift]);
#pragma unroll
    for (u32 m = 0; m < 7; ++m) {  // scalar loads; round 0 multiplies by w^128, w^256 (twice: m = 2 and 5) and w^384
      w1[m] = ld16(&W[(size_t)t4w_tw_index<3>(j1, m) << wshift]);
      if (m >= 4) w0[m] = ld16(&W[(size_t)t4w_tw_index<0>(0, m) << wshift]);
    }
#pragma unroll
    for (u32 m = 0; m < 7; ++m) {  // the empty asm keeps them here, all ten behind one wait: the compiler would sink them to their rounds
      asm volatile("" : "+s"(w1[m].lo), "+s"(w1[m].hi));
      if (m >= 4) asm volatile("" : "+s"(w0[m].lo), "+s"(w0[m].hi));
    }
    w0[2] = w0[5];
    __builtin_amdgcn_sched_barrier(0);  // every load in flight before the first wait, as in fp_fft_tile_1024x4
    if (KFAST_SRC) {
      if constexpr (T4IsIlp<O>::value) {
#pragma unroll
        for (u32 a = 0; a < 8; a += 2) T4Ops<O>::mul2_tw(y[a], t[a], y[a + 1], t[a + 1]);
      } else {
#pragma unroll
        for (u32 a = 0; a < 8; ++a) y[a] = T4Ops<O>::mul_tw(y[a], t[a]);
      }
    }
    t4w_round0<O>(s, y, kb, c, w0);
    st16(&wl[t4_wslot(tid)], wv);
  }
  __syncthreads();
  t4w_round1<O>(s, tid, j1, w1);
  __syncthreads();
#pragma unroll
  for (u32 g = 0; g < 2; ++g) t4w_round2<O>(s, tid + 512 * g, wl, W, wshift);
  __syncthreads();
  {  // round 3
    elt_t* dst = p.dst + (long long)by * p.dst_row + (long long)bx * p.dst_tile;
    const u32 dk = (u32)p.dk, dc = (u32)p.dc;
#pragma unroll
    for (u32 g = 0; g < 2; ++g) {
      const u32 e = tid + 512 * g, c = e & 3, j = e >> 2;
      elt_t x[4];
      t4w_round3_load(x, s, e);
      if constexpr (T4IsIlp<O>::value) t4i_stages4<O, 8, KFAST_SRC ? T4_LAZY_OUT : T4_LAZY>(x, j, wl);
      else t4_stages<O, 8, 2, false, KFAST_SRC ? T4_LAZY_OUT : T4_LAZY>(x, j, wl, W, wshift);
#pragma unroll
      for (u32 a = 0; a < 4; ++a) st16(dst + ((j + 256 * a) * dk + c * dc), x[a]);
    }
  }
}

// ------------------------------------------------------------------ K1: the 1024 x 4 pair without the address arithmetic
// fp_fft_tile_1024x4_lean is fp_fft_tile_1024x4_tw2<T4Ilp<O>, ..> with fewer VALU instructions that are not arithmetic: the same
// tile loads, values, LDS tile (layout (4p + c) ^ L(p)) and stores, the same products, canons and lazy butterflies in the same
// order.  The default for Fp128 where that pair was (LFGPU_FP_LEAN=0 launches it again).  It has round helpers of its own
// (t4l_*); DESIGN 4.1, profiles/k1_lean/.
//
// Global memory.  A tile's source, destination and (pass B) table slice are 64-bit bases in SGPRs and a thread's offsets are
// 32-bit byte offsets in VGPRs, the scalar-address form of global_load / global_store: no 64-bit vector arithmetic.  The step
// between a thread's eight points is uniform (128 sk elements on the load side, 128 dk between the two groups and 256 dk inside
// a group on the store side) and is added to the base on the scalar unit: eight bases, one offset.  Built the other way as well,
// one base and eight offsets (7 v_add_u32 per eight accesses): 21.20 against 21.17 ms per bench.py step, both below the 21.49 ms
// of fp_fft_tile_1024x4_tw2<T4Ilp<..>> (profiles/k1_lean/), so plain scalar adds cost no time that shows and the fewer VALU
// instructions stay.
// The 32 bits suffice because the host launches this pair only when a tile spans less than 2^32 bytes on both sides,
// 16 (1024 sk + 4 sc) and 16 (1024 dk + 4 dc) <= 2^32 - 1 (launch_tile_1024x4_tws), and every other plan goes to
// fp_fft_tile_1024x4_tw2.  The plans that reach the pair: pass A reads and writes rows of 2^20 points in columns of 4 (sk = dk =
// 1024, sc = dc = 1: 16 MiB); pass B reads 4 contiguous rows of 1024 points (64 KiB) and writes with dk = 1024 d, dc = d, where
// d = 1 for n = 2^20 and d = n / 2^20 <= 8 for the inner transforms of n = 2^21 .. 2^23 (16 MiB d <= 128 MiB; d >= 256, n >= 2^28,
// is refused).  A row stride ld > n enters only the 64-bit bases (by * src_row, by * dst_row).
//
// Tile order.  Pass A's column-block count is a power of two 2^lcb >= 8 (the host sends any other to fp_fft_tile_1024x4_tw2), so
// t4_xcd_order's quotient and remainder are shifts and masks of the workgroup index on the scalar unit.
//
// LDS.  Every address is a byte address computed once per thread and round, t4l_byte(p, c) = 16 ((4p + c) ^ L(p)), and the other
// slots of the round are that one XOR a constant plus an immediate offset; the kernel has no static LDS, so the tile starts at
// LDS address 0 and the addresses are plain integers.  With p = p0 + 2^k a and bit k of p0 clear, bit k moves (4p + c) by
// 64 2^k bytes, an immediate, and L(p) by 16 L(2^k), an XOR: L(64) = 4, L(128) = 9, L(256) = 2, L(512) = 4 (t4w_swz).
//   round 0: 8b + a, a < 8: a & 3 reaches slot bits 2-3 (XOR 64 (a & 3)), a >> 2 is + 256.
//   round 1: 64h + j + 8a with j uniform: j < 8 lies below every bit L reads, so the base is t4l_byte(64h, c) ^ 64 j, + 512 a.
//   round 2: 256h + j + 64a, h = h0 + 2g for group g: a moves p6, p7: XOR 16 L(64a) = {0, 64, 144, 208}, + 4096 a.  g moves p9:
//            + 32768 and XOR 64, and since {0, 64, 144, 208} ^ 64 is the same set, group 1 reuses group 0's four addresses.
//   round 3: j0 + 128g + 256a: a moves p8, p9: XOR 32 a, + 16384 a; g moves p7: XOR 144, + 8192.
// Stage twiddles of rounds 2 and 3, the one thing this pair keeps elsewhere in LDS: w_1024^i, i < 512, at byte T4L_W + 16 i with
// no swizzle, and behind them w_1024^(8j), j < 64, at T4L_W8 + 16 j (1 KiB more: 73 KiB per workgroup, two per CU).  Lanes walk c,
// then j, so the 16 lanes of a ds_read_b128 group read four consecutive j, four lanes each the same address.  Round 2 reads
// i = 8j from the second table (slots j .. j + 3) and i = 4j, 4j + 256 from the first (slots 4j .. 4j + 12, + 4096 bytes), the same
// for both groups; round 3 reads i = 2j, j, j + 256 with j = j0 + 128 g (slots 2j .. 2j + 6 and j .. j + 3; g is + 4096 and
// + 2048 bytes): distinct mod 16 in every group, which t4_wslot was there to achieve for the readers of the other kernels.  Two
// addresses per round, each a shift and a mask of tid, and immediates.  The first table is written as before, one entry per
// thread; wave 0 loads the 64 entries of the second beside the tile's loads and stores them on its own path of round 1.
__device__ __forceinline__ u32 t4l_byte(u32 p, u32 c) { return ((p << 6) | (c << 4)) ^ ((p >> 3) & 0x70u) ^ (p & 0xc0u); }  // 16 t4w_slot(p, c)
enum : u32 { T4L_W = 65536, T4L_W8 = T4L_W + 8192, T4L_LDS = T4L_W8 + 1024 };  // behind the tile; the workgroup's LDS bytes
typedef u32 t4l_v4 __attribute__((ext_vector_type(4)));  // a plain vector: uint4 is a class on the host pass
typedef __attribute__((address_space(3))) t4l_v4 t4l_lds_t;
__device__ __forceinline__ elt_t t4l_ld(u32 byte) {
  const t4l_v4 v = *(const t4l_lds_t*)(uintptr_t)byte;
  return elt_t{((u64)v.y << 32) | v.x, ((u64)v.w << 32) | v.z};
}
__device__ __forceinline__ void t4l_st(u32 byte, elt_t e) {
  const t4l_v4 v = {(u32)e.lo, (u32)(e.lo >> 32), (u32)e.hi, (u32)(e.hi >> 32)};
  *(t4l_lds_t*)(uintptr_t)byte = v;
}
// base + step + off in global memory for a uniform base and step
typedef __attribute__((address_space(1))) t4l_v4 t4l_glb_t;
__device__ __forceinline__ t4l_glb_t* t4l_at(const char* base, u32 step, u32 off) {
  u64 b = (u64)base + step;
  asm("" : "+s"(b));  // the sum stays on the scalar unit: left alone, the compiler adds step to base + off in VGPRs
  return (t4l_glb_t*)(b + off);
}
__device__ __forceinline__ elt_t t4l_gld(const t4l_glb_t* q) {
  const t4l_v4 v = *q;
  return elt_t{((u64)v.y << 32) | v.x, ((u64)v.w << 32) | v.z};
}
__device__ __forceinline__ void t4l_gst(t4l_glb_t* q, elt_t e) {
  const t4l_v4 v = {(u32)e.lo, (u32)(e.lo >> 32), (u32)e.hi, (u32)(e.hi >> 32)};
  *q = v;
}
// The three stages of rounds 0 and 1, as t4i_stage, with the butterflies that add in full (round 0) in pairs as well
template <class O, u32 MODE, u32 T>
__device__ __forceinline__ void t4l_stage(elt_t* x, const elt_t* w) {
  constexpr T4iStage S = t4i_plan<MODE>(T);
  constexpr u32 half = 1u << T, first = half - 1;
#pragma unroll
  for (u32 i = 0; i + 1 < S.np; i += 2) {
    const u32 a = S.prod[i], b = S.prod[i + 1];
    T4Ops<O>::mul2_tw_sw(x[a + half], w[first + (a & first)], x[b + half], w[first + (b & first)]);
  }
  if constexpr (S.np & 1) x[S.prod[S.np - 1] + half] = T4Ops<O>::mul_tw_sw(x[S.prod[S.np - 1] + half], w[first + (S.prod[S.np - 1] & first)]);
#pragma unroll
  for (u32 i = 0; i + 1 < S.nc; i += 2) T4Ops<O>::canon2(x[S.can[i] + half], x[S.can[i + 1] + half]);
  if constexpr (S.nc & 1) x[S.can[S.nc - 1] + half] = T4Ops<O>::canon(x[S.can[S.nc - 1] + half]);
#pragma unroll
  for (u32 i = 0; i + 1 < S.nf; i += 2) T4Ops<O>::bfly2_full(x[S.full[i]], x[S.full[i] + half], x[S.full[i + 1]], x[S.full[i + 1] + half]);
  if constexpr (S.nf & 1) {  // stage 0's third and stage 1's only one: the latter reads the former's result, they make no pair
    const u32 a = S.full[S.nf - 1];
    const elt_t u = x[a], v = x[a + half];
    x[a] = T4Ops<O>::add(u, v);
    x[a + half] = T4Ops<O>::sub(u, v);
  }
#pragma unroll
  for (u32 i = 0; i + 1 < S.nl; i += 2) T4Ops<O>::bfly2_lazy(x[S.lazy[i]], x[S.lazy[i] + half], x[S.lazy[i + 1]], x[S.lazy[i + 1] + half]);
  if constexpr (S.nl & 1) T4Ops<O>::bfly_lazy(x[S.lazy[S.nl - 1]], x[S.lazy[S.nl - 1] + half]);
}
template <class O, u32 MODE>
__device__ __forceinline__ void t4l_stages(elt_t* x, const elt_t* w) {
  t4l_stage<O, MODE, 0>(x, w);
  t4l_stage<O, MODE, 1>(x, w);
  t4l_stage<O, MODE, 2>(x, w);
}
// Rounds 2 and 3, as t4i_stages4, with the stage's three twiddles w^(2i), w^i, w^(i + 256) read by the caller; the two butterflies
// of T4_LAZY_OUT's last stage are one pair
template <class O, u32 LZ>
__device__ __forceinline__ void t4l_stages4(elt_t* x, elt_t w2, elt_t w1, elt_t w1h) {
  T4Ops<O>::mul2_tw(x[1], w2, x[3], w2);
  T4Ops<O>::bfly2_lazy(x[0], x[1], x[2], x[3]);
  T4Ops<O>::mul2_tw(x[2], w1, x[3], w1h);
  if (LZ == T4_LAZY_OUT) {
    T4Ops<O>::canon2(x[0], x[1]);
    T4Ops<O>::bfly2_full(x[0], x[2], x[1], x[3]);
  } else {
    T4Ops<O>::bfly2_lazy(x[0], x[2], x[1], x[3]);
  }
}
template <class O>
__device__ __forceinline__ void t4l_round0(const elt_t* y, u32 kb, u32 c, const elt_t* w) {
  elt_t x[8];
#pragma unroll
  for (u32 a = 0; a < 8; ++a) x[a] = y[((a & 1) << 2) | (a & 2) | (a >> 2)];
  t4l_stages<O, T4W_R0>(x, w);
  const u32 s0 = t4l_byte((__brev(kb) >> 25) << 3, c);
#pragma unroll
  for (u32 a = 0; a < 8; ++a) t4l_st((s0 ^ (64 * (a & 3))) + 256 * (a >> 2), x[a]);
}
template <class O, u32 MODE>
__device__ __forceinline__ void t4l_round1_wave(u32 s0, const elt_t* w) {
  elt_t x[8];
#pragma unroll
  for (u32 a = 0; a < 8; ++a) x[a] = t4l_ld(s0 + 512 * a);
  t4l_stages<O, MODE>(x, w);
#pragma unroll
  for (u32 a = 0; a < 8; ++a) t4l_st(s0 + 512 * a, x[a]);
}
// as t4w_round1: each path loads and stores for itself, the asm comments keep the compiler from merging them
template <class O>
__device__ __forceinline__ void t4l_round1(u32 tid, u32 j, const elt_t* w, elt_t w8) {
  const u32 s0 = t4l_byte(((tid >> 2) & 15) << 6, tid & 3) ^ (j << 6);
  if (j == 0) {
    t4l_st(T4L_W8 + (tid << 4), w8);  // wave 0: tid < 64
    asm volatile("; round 1, j = 0");
    t4l_round1_wave<O, T4W_R1_J0>(s0, w);
    asm volatile("; round 1, j = 0: stored");
  } else {
    asm volatile("; round 1, j > 0");
    t4l_round1_wave<O, T4W_R1>(s0, w);
    asm volatile("; round 1, j > 0: stored");
  }
}
// Round 2, both groups: the thread's four addresses serve group 0 in the order a and group 1, + 32768, in the order a ^ 1
template <class O>
__device__ __forceinline__ void t4l_round2(u32 tid) {
  const u32 j = (tid >> 2) & 63, s0 = t4l_byte(((tid >> 8) << 8) | j, tid & 3);
  const u32 sa[4] = {s0, s0 ^ 64, s0 ^ 144, s0 ^ 208};  // 16 L(64a) = 0, 64, 144, 208
  const u32 j16 = (tid << 2) & 0x3f0u;  // 16 j
  u32 wa = T4L_W8 + j16, wb = T4L_W + 4 * j16;
  asm("" : "+v"(wa), "+v"(wb));  // opaque, here and in round 3: + 4096 stays an immediate instead of a second address
  const elt_t w2 = t4l_ld(wa), w1 = t4l_ld(wb), w1h = t4l_ld(wb + 4096);
#pragma unroll
  for (u32 g = 0; g < 2; ++g) {
    elt_t x[4];
#pragma unroll
    for (u32 a = 0; a < 4; ++a) x[a] = t4l_ld(sa[a ^ g] + 4096 * a + 32768 * g);
    t4l_stages4<O, T4_LAZY>(x, w2, w1, w1h);
#pragma unroll
    for (u32 a = 0; a < 4; ++a) t4l_st(sa[a ^ g] + 4096 * a + 32768 * g, x[a]);
  }
}

template <class O, bool KFAST_SRC>
__global__ __launch_bounds__(512, 4) void fp_fft_tile_1024x4_lean(TilePlan p, const elt_t* __restrict__ W, u32 wshift,
                                                                  const elt_t* __restrict__ tw, u32 row_fast, u32 lcb) {
  const u32 tid = threadIdx.x, j1 = __builtin_amdgcn_readfirstlane(tid >> 6);
  u32 bx, by;  // (tile, batch row)
  if (KFAST_SRC) {
    bx = row_fast ? blockIdx.y : blockIdx.x;
    by = row_fast ? blockIdx.x : blockIdx.y;
  } else {  // t4_xcd_order for 2^lcb column blocks, lcb >= 3
    const u32 i = blockIdx.x >> 3, sh = lcb - 3;
    bx = ((blockIdx.x & 7) << sh) + (i & ((1u << sh) - 1));
    by = i >> sh;
  }
  elt_t w0[7] = {}, w1[7], wv8;  // the stage twiddles of rounds 0 and 1, and w^(8 lane)
  {  // round 0
    const u32 c = KFAST_SRC ? tid >> 7 : tid & 3, kb = KFAST_SRC ? tid & 127 : tid >> 2;
    const char* src = (const char*)(p.src + (long long)by * p.src_row + (long long)bx * p.src_tile);
    const u32 sk = (u32)p.sk << 4, off = kb * sk + c * ((u32)p.sc << 4);
    elt_t y[8], t[8];
#pragma unroll
    for (u32 a = 0; a < 8; ++a) y[a] = t4l_gld(t4l_at(src, 128 * a * sk, off));
    if (KFAST_SRC) {
      const char* twt = (const char*)(tw + ((size_t)bx << 12));
      const u32 toff = ((c << 10) + kb) << 4;
#pragma unroll
      for (u32 a = 0; a < 8; ++a) t[a] = t4l_gld(t4l_at(twt, 2048 * a, toff));
    }
    const elt_t wv = t4l_gld(t4l_at((const char*)W, 0, tid << (wshift + 4)));
    wv8 = t4l_gld(t4l_at((const char*)W, 0, (tid & 63) << (wshift + 7)));  // w^(8 lane): wave 0 keeps it
#pragma unroll
    for (u32 m = 0; m < 7; ++m) {  // scalar loads, as fp_fft_tile_1024x4_tw2
      w1[m] = ld16(&W[(size_t)t4w_tw_index<3>(j1, m) << wshift]);
      if (m >= 4) w0[m] = ld16(&W[(size_t)t4w_tw_index<0>(0, m) << wshift]);
    }
#pragma unroll
    for (u32 m = 0; m < 7; ++m) {
      asm volatile("" : "+s"(w1[m].lo), "+s"(w1[m].hi));
      if (m >= 4) asm volatile("" : "+s"(w0[m].lo), "+s"(w0[m].hi));
    }
    w0[2] = w0[5];
    __builtin_amdgcn_sched_barrier(0);  // every load in flight before the first wait
    if (KFAST_SRC) {
#pragma unroll
      for (u32 a = 0; a < 8; a += 2) T4Ops<O>::mul2_tw(y[a], t[a], y[a + 1], t[a + 1]);
    }
    t4l_round0<O>(y, kb, c, w0);
    asm volatile("" ::"v"(wv8.lo), "v"(wv8.hi));  // loaded here, beside wv: the compiler would move the load to wave 0's path of round 1
    t4l_st(T4L_W + (tid << 4), wv);
  }
  __syncthreads();
  t4l_round1<O>(tid, j1, w1, wv8);
  __syncthreads();
  t4l_round2<O>(tid);
  __syncthreads();
  {  // round 3: group g holds j = j0 + 128 g, its outputs the points j + 256 a
    char* dst = (char*)(p.dst + (long long)by * p.dst_row + (long long)bx * p.dst_tile);
    const u32 j0 = tid >> 2, c = tid & 3, dk = (u32)p.dk << 4, off = j0 * dk + c * ((u32)p.dc << 4);
    const u32 s0 = t4l_byte(j0, c);
    u32 wa = T4L_W + ((tid << 3) & ~31u), wb = T4L_W + ((tid << 2) & ~15u);  // w^(2 j0), w^j0
    asm("" : "+v"(wa), "+v"(wb));
#pragma unroll
    for (u32 g = 0; g < 2; ++g) {
      const u32 sg = g ? s0 ^ 144 : s0;
      elt_t x[4];
#pragma unroll
      for (u32 a = 0; a < 4; ++a) x[a] = t4l_ld((sg ^ (32 * a)) + 16384 * a + 8192 * g);
      const elt_t w2 = t4l_ld(wa + 4096 * g), w1s = t4l_ld(wb + 2048 * g), w1h = t4l_ld(wb + 2048 * g + 4096);
      t4l_stages4<O, KFAST_SRC ? T4_LAZY_OUT : T4_LAZY>(x, w2, w1s, w1h);
#pragma unroll
      for (u32 a = 0; a < 4; ++a) t4l_gst(t4l_at(dst, (128 * g + 256 * a) * dk, off), x[a]);
    }
  }
}

// ------------------------------------------------------------------ K2: LCH14
// Stage ii of the tile (global stage i = i_lo + ii) uses
//   tw = tbl[off[ii] + u_local]  (^ base[ii*nb + cbase + c] when base != null)
// fwd (lch14.h:219-223): b0 ^= tw*b1; b1 ^= b0.   bwd (:225-229): b1 ^= b0; b0 ^= tw*b1.
struct LchTables {
  const elt_t* tbl;
  const elt_t* base;
  u32 nb;
  u32 off[16];
};

template <int FFT_THREADS>
__global__ __launch_bounds__(FFT_THREADS) void lch_fft_tile(TilePlan p, int inverse, LchTables t) {
  extern __shared__ elt_t s[];
  const u32 T = 1u << p.logT, C = 1u << p.logC, tid = threadIdx.x;
  const u32 cbase = blockIdx.x << p.logC;
  const elt_t* src = p.src + (long long)blockIdx.y * p.src_row + (long long)blockIdx.x * p.src_tile;
  elt_t* dst = p.dst + (long long)blockIdx.y * p.dst_row + (long long)blockIdx.x * p.dst_tile;

  for (u32 e = tid; e < T * C; e += FFT_THREADS) {
    u32 k, c;
    if (p.kfast_src) { k = e & (T - 1); c = e >> p.logT; } else { c = e & (C - 1); k = e >> p.logC; }
    elt_t v = elt_zero();
    if (cbase + c < p.nbatch) v = ld16(src + (long long)k * p.sk + (long long)c * p.sc);
    st16(&s[(k << p.logC) + c], v);
  }
  __syncthreads();
  for (u32 step = 0; step < p.logT; ++step) {
    const u32 ii = inverse ? step : (p.logT - 1 - step);
    const u32 sz = 1u << ii;
    for (u32 e = tid; e < (T >> 1) * C; e += FFT_THREADS) {
      u32 c = e & (C - 1), b = e >> p.logC;
      u32 v = b & (sz - 1), u = b >> ii;
      u32 i0 = (u << (ii + 1)) + v, i1 = i0 + sz;
      elt_t tw = ld16(&t.tbl[t.off[ii] + u]);
      if (t.base) {
        u32 cb = cbase + c;
        if (cb >= t.nb) cb = 0;
        tw = gf_add(tw, ld16(&t.base[ii * t.nb + cb]));
      }
      elt_t b0 = ld16(&s[(i0 << p.logC) + c]);
      elt_t b1 = ld16(&s[(i1 << p.logC) + c]);
      if (!inverse) {
        b0 = gf_add(b0, gf_mul(tw, b1));
        b1 = gf_add(b1, b0);
      } else {
        b1 = gf_add(b1, b0);
        b0 = gf_add(b0, gf_mul(tw, b1));
      }
      st16(&s[(i0 << p.logC) + c], b0);
      st16(&s[(i1 << p.logC) + c], b1);
    }
    __syncthreads();
  }
  for (u32 e = tid; e < T * C; e += FFT_THREADS) {
    u32 j, c;
    if (p.kfast_dst) { j = e & (T - 1); c = e >> p.logT; } else { c = e & (C - 1); j = e >> p.logC; }
    if (cbase + c >= p.nbatch) continue;
    st16(dst + (long long)j * p.dk + (long long)c * p.dc, ld16(&s[(j << p.logC) + c]));
  }
}

// ------------------------------------------------------------------ host side
template <class O>
static int set_lds_limit_fp(lfgpu_ctx* c) {
  LF_HIP(c, hipFuncSetAttribute((const void*)fp_fft_tile<O, 1024, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  LF_HIP(c, hipFuncSetAttribute((const void*)fp_fft_tile<O, 1024, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  LF_HIP(c, hipFuncSetAttribute((const void*)fp_fft_tile<O, 512, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  LF_HIP(c, hipFuncSetAttribute((const void*)fp_fft_tile<O, 512, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return LFGPU_OK;
}
static int set_lds_limit(lfgpu_ctx* c) {
  if (!(c->attr_done & 1u)) {
    if (const char* e = getenv("LFGPU_TILE_LOG")) {  // tuning knob: 12 or 13
      int v = atoi(e);
      if (v == 12 || v == 13) c->tile_log = v;
    }
    LF_TRY(set_lds_limit_fp<Fp128Ops>(c));
    const void* const t4[] = {(const void*)fp_fft_tile_1024x4<Fp128Ops, false, true>,
                              (const void*)fp_fft_tile_1024x4<Fp128Ops, true, false>,
                              (const void*)fp_fft_tile_1024x4_persist<Fp128Ops>,
                              (const void*)fp_fft_tile_1024x4_tws<Fp128Ops, false>,
                              (const void*)fp_fft_tile_1024x4_tws<Fp128Ops, true>,
                              (const void*)fp_fft_tile_1024x4_tws_canon<Fp128Ops, false>,
                              (const void*)fp_fft_tile_1024x4_tws_canon<Fp128Ops, true>,
                              (const void*)fp_fft_tile_1024x4_tw2<Fp128Ops, false>,
                              (const void*)fp_fft_tile_1024x4_tw2<Fp128Ops, true>,
                              (const void*)fp_fft_tile_1024x4_tw2<T4Ilp<Fp128Ops>, false>,
                              (const void*)fp_fft_tile_1024x4_tw2<T4Ilp<Fp128Ops>, true>,
                              (const void*)fp_fft_tile_1024x4_lean<T4Ilp<Fp128Ops>, false>,
                              (const void*)fp_fft_tile_1024x4_lean<T4Ilp<Fp128Ops>, true>};
    for (const void* k : t4) LF_HIP(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    LF_TRY(set_lds_limit_fp<F64x2Ops<true>>(c));
    LF_TRY(set_lds_limit_fp<F64x2Ops<false>>(c));
    LF_HIP(c, hipFuncSetAttribute((const void*)lch_fft_tile<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, TILE_ELTS * 16));
    LF_HIP(c, hipFuncSetAttribute((const void*)lch_fft_tile<512>, hipFuncAttributeMaxDynamicSharedMemorySize, TILE_ELTS * 16));
    c->attr_done |= 1u;
  }
  return LFGPU_OK;
}

// LDS of one Fp128 tile: the elements, plus the T/2 stage twiddles when both fit (p.wlds)
static size_t fp_lds_bytes(TilePlan& p) {
  const size_t tile = ((size_t)16 << p.logT) << p.logC, tw = (size_t)8 << p.logT;
  p.wlds = tile + tw <= 160u * 1024u ? 1u : 0u;
  return p.wlds ? tile + tw : tile;
}
template <class O, class... Args>
static void launch_fp(lfgpu_ctx* c, dim3 grid, size_t lds, const TilePlan& p, Args... args) {
  if (c->tile_log == 13) {
    if (p.wlds) hipLaunchKernelGGL((fp_fft_tile<O, 1024, true>), grid, dim3(1024), lds, c->stream, p, args...);
    else hipLaunchKernelGGL((fp_fft_tile<O, 1024, false>), grid, dim3(1024), lds, c->stream, p, args...);
  } else {
    if (p.wlds) hipLaunchKernelGGL((fp_fft_tile<O, 512, true>), grid, dim3(512), lds, c->stream, p, args...);
    else hipLaunchKernelGGL((fp_fft_tile<O, 512, false>), grid, dim3(512), lds, c->stream, p, args...);
  }
}
// The LFGPU_FP_* switches of K1, all read once per process, at the first transform.
struct FpSwitches {
  bool tile1024;    // LFGPU_FP_TILE1024 (default 1): 0 keeps every tile on the generic fp_fft_tile
  int persist;      // LFGPU_FP_PERSIST (default 1): see launch_tile_1024x4_persist
  int twside;       // LFGPU_FP_TWSIDE (default 1): see fp_twside_mode
  bool other_plan;  // LFGPU_FP_PERSIST or LFGPU_FP_TILE1024 is set at all, to whatever value
  bool lazy;        // LFGPU_FP_LAZY (default 1): 0 launches fp_fft_tile_1024x4_tws_canon
  bool r1wave;      // LFGPU_FP_R1WAVE (default 1): 0 launches fp_fft_tile_1024x4_tws where the wave-uniform round 1 is the default
  bool ilp;         // LFGPU_FP_ILP (default 1): 0 launches fp_fft_tile_1024x4_tw2 where fp_fft_tile_1024x4_ilp is the default
  bool lean;        // LFGPU_FP_LEAN (default 1): 0 launches fp_fft_tile_1024x4_ilp where fp_fft_tile_1024x4_lean is the default
  bool two_level;   // LFGPU_FP_TW=2: the two-level inter-pass table
  bool row_fast;    // LFGPU_FP_ROWFAST (default 1): 0 keeps pass A's tiles fastest in the grid
};
static const FpSwitches& fp_switches() {
  static const FpSwitches sw = [] {
    const auto num = [](const char* name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; };
    FpSwitches w;
    w.tile1024 = num("LFGPU_FP_TILE1024", 1) != 0;
    w.persist = num("LFGPU_FP_PERSIST", 1);
    w.twside = num("LFGPU_FP_TWSIDE", 1);
    w.other_plan = getenv("LFGPU_FP_PERSIST") || getenv("LFGPU_FP_TILE1024");
    w.lazy = num("LFGPU_FP_LAZY", 1) != 0;
    w.r1wave = num("LFGPU_FP_R1WAVE", 1) != 0;
    w.ilp = num("LFGPU_FP_ILP", 1) != 0;
    w.lean = num("LFGPU_FP_LEAN", 1) != 0;
    w.two_level = num("LFGPU_FP_TW", 0) == 2;
    w.row_fast = num("LFGPU_FP_ROWFAST", 1) != 0;
    return w;
  }();
  return sw;
}
// Is the plan a tile of the 1024 x 4 kernels (pass B with kfast_src, pass A without)?  offsets32: also every offset inside a
// tile, on the load and the store side, non-negative and in 32 bits, as _persist and _tws compute them.
static bool tile_1024x4_fits(const TilePlan& p, bool kfast_src, bool offsets32) {
  if (p.logT != 10 || p.logC != 2 || !p.wlds || p.kfast_src != (kfast_src ? 1u : 0u) || p.kfast_dst != 0 || (p.nbatch & 3) != 0) return false;
  return !offsets32 || (p.sk >= 0 && p.sc >= 0 && p.dk >= 0 && p.dc >= 0 && (u64)p.sk * 1024 + (u64)p.sc * 4 <= 0xffffffffu &&
                        (u64)p.dk * 1024 + (u64)p.dc * 4 <= 0xffffffffu);
}
// May a plan that fits fp_fft_tile_1024x4_tw2 go to fp_fft_tile_1024x4_lean?  Its offsets inside a tile are 32-bit byte offsets, so
// a tile spans less than 2^32 bytes on the load and the store side (and the stage-twiddle table, 512 entries 2^wshift apart); its
// tile order wants the column-block count a power of two, in pass A with 8 or more blocks.  *lcb: log2 of that count.
static bool tile_1024x4_lean_fits(const TilePlan& p, bool kfast_src, u32 wshift, u32* lcb) {
  const u32 ncb = p.nbatch >> 2;
  if (ncb == 0 || (ncb & (ncb - 1)) != 0 || (!kfast_src && ncb < 8) || wshift > 16) return false;
  if (((u64)p.sk * 1024 + (u64)p.sc * 4) * 16 > 0xffffffffu || ((u64)p.dk * 1024 + (u64)p.dc * 4) * 16 > 0xffffffffu) return false;
  *lcb = lf_log2(ncb);
  return true;
}
// Pass A through fp_fft_tile_1024x4_persist.  LFGPU_FP_PERSIST: 0 = fp_fft_tile_1024x4 in the grid order of the caller, 1 (default)
// = one tile per workgroup in the XCD-aware tile order, 2 = the tile loop on as many workgroups as the CUs hold at once (measured
// slower than 1: 29.7 against 28.1 ms per bench.py step).  Returns false, launching nothing, for 0.
template <class O>
static bool launch_tile_1024x4_persist(lfgpu_ctx* c, u32 rows, size_t lds, const TilePlan& p, const elt_t* W, u32 wshift, const elt_t* tw) {
  const int mode = fp_switches().persist;
  const u32 ncb = p.nbatch >> 2;
  u32 parts = rows;
  if (mode <= 0 || !tile_1024x4_fits(p, false, true)) return false;
  if (mode >= 2) {
    static const int per_cu = [lds] {  // 2: LDS (2 x 72 KiB) and VGPRs (<= 128) both allow two workgroups per CU
      int n = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)fp_fft_tile_1024x4_persist<O>, 512, lds) != hipSuccess)
        n = 0;
      return n < 1 ? 1 : n;
    }();
    const u32 fill = (u32)per_cu * (u32)c->num_cu;
    parts = fill / ncb;
    if (parts < 1) parts = 1;
    if (parts > rows) parts = rows;
  }
  if ((u64)ncb * parts > 0x7fffffffu) return false;
  const dim3 grid(ncb * parts);
  hipLaunchKernelGGL((fp_fft_tile_1024x4_persist<O>), grid, dim3(512), lds, c->stream, p, W, wshift, tw, rows, parts);
  return true;
}
// fp_fft_tile_1024x4 takes an Fp128 tile of 1024 x 4 in the 512-thread configuration; LFGPU_FP_TILE1024=0 keeps every tile on
// the generic fp_fft_tile (returns false, launching nothing, otherwise)
template <class O, bool KFAST_SRC, bool TW>
static bool launch_tile_1024x4(lfgpu_ctx* c, dim3 grid, size_t lds, const TilePlan& p, const elt_t* W, u32 wshift, const elt_t* tw,
                               u32 row_fast) {
  if constexpr (std::is_same<O, Fp128Ops>::value) {
    if (fp_switches().tile1024 && c->tile_log == 12 && tile_1024x4_fits(p, KFAST_SRC, false)) {
      if constexpr (!KFAST_SRC && TW)
        if (launch_tile_1024x4_persist<O>(c, row_fast ? grid.x : grid.y, lds, p, W, wshift, tw)) return true;
      hipLaunchKernelGGL((fp_fft_tile_1024x4<O, KFAST_SRC, TW>), grid, dim3(512), lds, c->stream, p, W, wshift, tw, row_fast);
      return true;
    }
  }
  return false;
}
// The pair fp_fft_tile_1024x4_tws (inter-pass product on pass B's load side): the default for Fp128 when both passes are 1024 x 4
// tiles (n = 2^20) and the full table is in use.  LFGPU_FP_TWSIDE=0, or any setting of LFGPU_FP_PERSIST or LFGPU_FP_TILE1024 (which
// choose among the kernels of the other plan), keeps the product in pass A; =2 runs pass B with the rows fastest in the grid.
// LFGPU_FP_LAZY=0 launches the pair with canonical butterflies, fp_fft_tile_1024x4_tws_canon, for both passes; otherwise the pair
// is fp_fft_tile_1024x4_lean (round 1 wave-uniform, arithmetic in pairs, scalar bases and byte addresses) for every plan it takes
// (tile_1024x4_lean_fits); LFGPU_FP_LEAN=0, and any other plan, launches fp_fft_tile_1024x4_ilp (the same values with the address
// arithmetic of fp_fft_tile_1024x4_tw2), LFGPU_FP_ILP=0 puts fp_fft_tile_1024x4_tw2 back (the same without the pairs) and
// LFGPU_FP_R1WAVE=0 fp_fft_tile_1024x4_tws.  None of the switches has an effect where this plan is not taken.
template <class O>
static int fp_twside_mode(const lfgpu_ctx* c, u32 logn1, size_t rows, bool two_level) {
  const int mode = fp_switches().other_plan ? 0 : fp_switches().twside;
  if (!std::is_same<O, Fp128Ops>::value || two_level || c->tile_log != 12 || logn1 != 10 || rows > (0x7fffffffu >> 8)) return 0;
  return mode < 0 ? 0 : mode;
}
// one pass of the pair; false, launching nothing, when the plan is not a 1024 x 4 tile with 32-bit offsets
template <class O, bool KFAST_SRC>
static bool launch_tile_1024x4_tws(lfgpu_ctx* c, u32 rows, size_t lds, const TilePlan& p, const elt_t* W, u32 wshift, const elt_t* tw,
                                   u32 row_fast) {
  if constexpr (std::is_same<O, Fp128Ops>::value) {
    const u32 ncb = p.nbatch >> 2;
    if (!tile_1024x4_fits(p, KFAST_SRC, true) || (u64)ncb * rows > 0x7fffffffu) return false;
    if (KFAST_SRC && (p.sk != 1 || p.sc != 1024 || p.src_tile != 4096)) return false;  // the table's layout [j1][k2]
    if (KFAST_SRC && (row_fast ? ncb : rows) > 65535) row_fast = !row_fast;
    const dim3 grid = !KFAST_SRC ? dim3(ncb * rows) : row_fast ? dim3(rows, ncb) : dim3(ncb, rows);
    u32 lcb = 0;
    if (!fp_switches().lazy) hipLaunchKernelGGL((fp_fft_tile_1024x4_tws_canon<O, KFAST_SRC>), grid, dim3(512), lds, c->stream, p, W, wshift, tw, row_fast);
    else if (fp_switches().r1wave && fp_switches().ilp && fp_switches().lean && tile_1024x4_lean_fits(p, KFAST_SRC, wshift, &lcb))
      hipLaunchKernelGGL((fp_fft_tile_1024x4_lean<T4Ilp<O>, KFAST_SRC>), grid, dim3(512), T4L_LDS, c->stream, p, W, wshift, tw, row_fast, lcb);
    else if (fp_switches().r1wave && fp_switches().ilp) hipLaunchKernelGGL((fp_fft_tile_1024x4_tw2<T4Ilp<O>, KFAST_SRC>), grid, dim3(512), lds, c->stream, p, W, wshift, tw, row_fast);
    else if (fp_switches().r1wave) hipLaunchKernelGGL((fp_fft_tile_1024x4_tw2<O, KFAST_SRC>), grid, dim3(512), lds, c->stream, p, W, wshift, tw, row_fast);
    else hipLaunchKernelGGL((fp_fft_tile_1024x4_tws<O, KFAST_SRC>), grid, dim3(512), lds, c->stream, p, W, wshift, tw, row_fast);
    return true;
  }
  return false;
}
template <class... Args>
static void launch_lch(lfgpu_ctx* c, dim3 grid, size_t lds, Args... args) {
  if (c->tile_log == 13)
    hipLaunchKernelGGL(lch_fft_tile<1024>, grid, dim3(1024), lds, c->stream, args...);
  else
    hipLaunchKernelGGL(lch_fft_tile<512>, grid, dim3(512), lds, c->stream, args...);
}

template <class O>
static elt_t fp_reroot(elt_t w, u64 n, u64 r) {  // twiddle.h:47-55
  while (r < n) {
    w = O::hmul(w, w);
    r += r;
  }
  return w;
}

static std::string keyf(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return std::string(buf);
}

// single-pass plan: T = n points, batch = rows
static TilePlan plan_single(const lfgpu_ctx* c, void* A, size_t rows, u32 logn, size_t ld) {
  TilePlan p{};
  u32 logC = (u32)c->tile_log - logn;
  u32 need = lf_log2(rows);
  if (logC > need) logC = need;
  p.src = (const elt_t*)A;
  p.dst = (elt_t*)A;
  p.src_row = p.dst_row = 0;
  p.src_tile = p.dst_tile = (long long)ld << logC;
  p.sk = p.dk = 1;
  p.sc = p.dc = (long long)ld;
  p.logT = logn;
  p.logC = logC;
  p.nbatch = (u32)rows;
  p.kfast_src = p.kfast_dst = 1;
  return p;
}

// root table W[i] = w_Tw^i, i < Tw/2, for a transform of 2^logn points with the root wn of that order
template <class O>
static int fp_root_table(lfgpu_ctx* c, const elt_t wn, u32 logn, u32 logTw, std::string* key_out, void** dW) {
  const size_t n = (size_t)1 << logn;
  std::string key = keyf("%sW:%llx:%llx:%u:%u", O::kKey, (u64)wn.lo, (u64)wn.hi, logn, logTw);
  if (!lf_table_lookup(c, key, dW)) {
    std::vector<elt_t> W((size_t)1 << (logTw ? logTw - 1 : 0));
    elt_t wt = fp_reroot<O>(wn, n, (u64)1 << logTw), x = O::one();
    for (size_t i = 0; i < W.size(); ++i) {
      W[i] = x;
      x = O::hmul(x, wt);
    }
    LF_TRY(lf_table(c, key, W.data(), W.size() * 16, dW));
  }
  *key_out = key;
  return LFGPU_OK;
}
// the two-level inter-pass table lo[e & 1023] = wn^(e & 1023), hi[e >> 10] = wn^(1024 (e >> 10)), e < n
template <class O>
static int fp_two_level_tables(lfgpu_ctx* c, const elt_t wn, u32 logn, const std::string& key, void** dlo, void** dhi) {
  std::string klo = key + ":lo", khi = key + ":hi";
  if (!lf_table_lookup(c, klo, dlo) || !lf_table_lookup(c, khi, dhi)) {
    std::vector<elt_t> lo(1024), hi((size_t)1 << (logn > 10 ? logn - 10 : 0));
    elt_t x = O::one();
    for (size_t i = 0; i < 1024; ++i) {
      lo[i] = x;
      x = O::hmul(x, wn);
    }
    elt_t w1024 = x;  // wn^1024
    x = O::one();
    for (size_t i = 0; i < hi.size(); ++i) {
      hi[i] = x;
      x = O::hmul(x, w1024);
    }
    LF_TRY(lf_table(c, klo, lo.data(), lo.size() * 16, dlo));
    LF_TRY(lf_table(c, khi, hi.data(), hi.size() * 16, dhi));
  }
  return LFGPU_OK;
}

// Two tile passes for 2^12 < n <= 2^20: `rows` transforms with the root wn of order n, row r read at src + r*sld and
// written to X[j] = dst[r*drow + j*dstep] (dstep = 1, drow = ld: a plain row).  Goes through `scratch`.
template <class O>
static int fp_fft_two_pass(lfgpu_ctx* c, const elt_t wn, u32 logn, size_t rows, const elt_t* src, size_t sld, elt_t* dst, long long drow,
                           long long dstep) {
  const size_t n = (size_t)1 << logn;
  const u32 logn2 = 10, logn1 = logn - logn2;
  const u32 logTw = logn1 > logn2 ? logn1 : logn2;  // root table covers the larger tile
  void *dW = nullptr, *dlo = nullptr, *dhi = nullptr;
  std::string key;
  LF_TRY(fp_root_table<O>(c, wn, logn, logTw, &key, &dW));
  // Inter-pass twiddles w_n^(j1*k2): either the full [j1][k2] table (n elements, default: one product
  // per element, table slices stay in L2 because batch rows vary fastest in the grid) or, with LFGPU_FP_TW=2, the
  // two-level form lo[e & 1023] * hi[e >> 10] (2 KiB + n/64 bytes of tables, two products per element).
  const bool two_level = fp_switches().two_level;
  const size_t n1 = (size_t)1 << logn1, n2 = (size_t)1 << logn2;
  if (two_level) {
    LF_TRY(fp_two_level_tables<O>(c, wn, logn, key, &dlo, &dhi));
  } else {
    std::string kfull = key + ":full";
    if (!lf_table_lookup(c, kfull, &dlo)) {
      std::vector<elt_t> full(n1 * n2);
      elt_t wj = O::one();  // wn^j1
      for (size_t j = 0; j < n1; ++j) {
        elt_t x = O::one();
        elt_t* row = &full[j * n2];
        for (size_t k = 0; k < n2; ++k) {
          row[k] = x;
          x = O::hmul(x, wj);
        }
        wj = O::hmul(wj, wn);
      }
      LF_TRY(lf_table(c, kfull, full.data(), full.size() * 16, &dlo));
    }
    dhi = nullptr;
  }
  void* scratch = nullptr;
  LF_TRY(lf_scratch(c, rows * n * 16, &scratch));
  const int twside = fp_twside_mode<O>(c, logn1, rows, two_level);  // the inter-pass product: in pass B (default at n = 2^20), or in pass A
  {  // pass A: n1-point transforms over k1 (stride n2), C consecutive k2 per tile
    TilePlan p{};
    p.logT = logn1;
    p.logC = (u32)c->tile_log - logn1;
    if (p.logC > logn2) p.logC = logn2;
    p.src = src;
    p.dst = (elt_t*)scratch;
    p.src_row = (long long)sld;
    p.dst_row = (long long)n;
    p.src_tile = p.dst_tile = 1ll << p.logC;
    p.sk = p.dk = (long long)n2;
    p.sc = p.dc = 1;
    p.nbatch = (u32)n2;
    p.kfast_src = p.kfast_dst = 0;
    size_t lds = fp_lds_bytes(p);
    // rows fastest: the tile's table slice is reused by every row while it is hot
    const u32 row_fast = (!two_level && rows <= 65535 && fp_switches().row_fast) ? 1u : 0u;
    const dim3 grid = row_fast ? dim3((u32)rows, (u32)(n2 >> p.logC)) : dim3((u32)(n2 >> p.logC), (u32)rows);
    if (twside) {
      if (!launch_tile_1024x4_tws<O, false>(c, (u32)rows, lds, p, (const elt_t*)dW, logTw - logn1, (const elt_t*)nullptr, 0u))
        return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "fp_fft: pass A does not fit the 1024 x 4 tile");
    } else if (two_level || !launch_tile_1024x4<O, false, true>(c, grid, lds, p, (const elt_t*)dW, logTw - logn1, (const elt_t*)dlo, row_fast))
      launch_fp<O>(c, grid, lds, p, (const elt_t*)dW, logTw - logn1, (const elt_t*)dlo, (const elt_t*)dhi, row_fast);
    LF_HIP(c, hipGetLastError());
  }
  {  // pass B: n2-point transforms on contiguous rows j1; output X[j1 + n1*j2]
    TilePlan p{};
    p.logT = logn2;
    p.logC = (u32)c->tile_log - logn2;
    if (p.logC > logn1) p.logC = logn1;
    p.src = (const elt_t*)scratch;
    p.dst = dst;
    p.src_row = (long long)n;
    p.dst_row = drow;
    p.src_tile = (long long)n2 << p.logC;
    p.dst_tile = (1ll << p.logC) * dstep;
    p.sk = 1;
    p.sc = (long long)n2;
    p.dk = (long long)n1 * dstep;
    p.dc = dstep;
    p.nbatch = (u32)n1;
    p.kfast_src = 1;
    p.kfast_dst = 0;
    size_t lds = fp_lds_bytes(p);
    const dim3 grid((u32)(n1 >> p.logC), (u32)rows);
    if (twside) {
      if (!launch_tile_1024x4_tws<O, true>(c, (u32)rows, lds, p, (const elt_t*)dW, logTw - logn2, (const elt_t*)dlo, twside == 2 ? 1u : 0u))
        return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "fp_fft: pass B does not fit the 1024 x 4 tile");
    } else if (!launch_tile_1024x4<O, true, false>(c, grid, lds, p, (const elt_t*)dW, logTw - logn2, (const elt_t*)nullptr, 0u))
      launch_fp<O>(c, grid, lds, p, (const elt_t*)dW, logTw - logn2, (const elt_t*)nullptr, (const elt_t*)nullptr, 0u);
    LF_HIP(c, hipGetLastError());
  }
  return LFGPU_OK;
}

// FFT<Field>::fftb / fftf (fft.h:185-201) for the field O describes
template <class O>
static int fft_any(lfgpu_ctx* c, const char* what, int dir, size_t rows, size_t n, const uint64_t omega[2], uint64_t omega_order, void* d_A,
                   size_t ld) {
  if (!c || !omega || (!d_A && rows && n)) return lf_fail(c, LFGPU_ERR_ARG, "%s: null argument", what);
  if (rows == 0 || n <= 1) return LFGPU_OK;
  if (n & (n - 1)) return lf_fail(c, LFGPU_ERR_ARG, "%s: n=%zu is not a power of two", what, n);
  if (omega_order < n || (omega_order & (omega_order - 1)))
    return lf_fail(c, LFGPU_ERR_ARG, "%s: omega_order must be a power of two >= n", what);
  if (ld < n) return lf_fail(c, LFGPU_ERR_ARG, "%s: ld < n", what);
  if (rows > 0x7fffffffu) return lf_fail(c, LFGPU_ERR_ARG, "%s: too many rows", what);
  const u32 logn = lf_log2(n);
  if (logn > 30) return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "%s: n > 2^30", what);
  LF_HIP(c, hipSetDevice(c->device));
  LF_TRY(set_lds_limit(c));

  elt_t w{omega[0], omega[1]};
  if (dir == 1) w = O::inv(w);  // fftf = fftb with omega^-1 (fft.h:198-201)
  elt_t wn = fp_reroot<O>(w, omega_order, n);
  if (logn <= (u32)c->tile_log) {  // one pass
    void* dW = nullptr;
    std::string key;
    LF_TRY(fp_root_table<O>(c, wn, logn, logn, &key, &dW));
    TilePlan p = plan_single(c, d_A, rows, logn, ld);
    u32 ntiles = (u32)((rows + (1u << p.logC) - 1) >> p.logC);
    size_t lds = fp_lds_bytes(p);
    launch_fp<O>(c, dim3(ntiles, 1), lds, p, (const elt_t*)dW, 0u, (const elt_t*)nullptr, (const elt_t*)nullptr, 0u);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  if (logn <= 20) return fp_fft_two_pass<O>(c, wn, logn, rows, (const elt_t*)d_A, ld, (elt_t*)d_A, (long long)ld, 1);
  // n > 2^20: n = n1 * 2^20.  Per row: one tile pass of n1-point transforms down the stride-2^20 dimension, multiplied by
  // the twiddles w_n^(j1 * column) (two-level table), written as n1 contiguous sequences of 2^20 points; those are
  // transformed by the two-pass plan with the root w_n^n1 and written to X[j1 + n1 * J].
  const u32 logn1 = logn - 20;
  const size_t n1 = (size_t)1 << logn1, n2 = (size_t)1 << 20;
  void *dW = nullptr, *dlo = nullptr, *dhi = nullptr, *mid = nullptr;
  std::string key;
  LF_TRY(fp_root_table<O>(c, wn, logn, logn1, &key, &dW));
  LF_TRY(fp_two_level_tables<O>(c, wn, logn, key, &dlo, &dhi));
  LF_TRY(lf_scratch2(c, n * 16, &mid));
  elt_t wi = wn;  // w_n^n1: the root of order 2^20 of the inner transforms
  for (u32 i = 0; i < logn1; ++i) wi = O::hmul(wi, wi);
  for (size_t r = 0; r < rows; ++r) {
    elt_t* row = (elt_t*)d_A + r * ld;
    TilePlan p{};
    p.logT = logn1;
    p.logC = (u32)c->tile_log - logn1;
    p.src = row;
    p.dst = (elt_t*)mid;
    p.src_row = p.dst_row = 0;
    p.src_tile = p.dst_tile = 1ll << p.logC;
    p.sk = p.dk = (long long)n2;
    p.sc = p.dc = 1;
    p.nbatch = (u32)n2;
    p.kfast_src = p.kfast_dst = 0;
    size_t lds = fp_lds_bytes(p);
    launch_fp<O>(c, dim3((u32)(n2 >> p.logC), 1), lds, p, (const elt_t*)dW, 0u, (const elt_t*)dlo, (const elt_t*)dhi, 0u);
    LF_HIP(c, hipGetLastError());
    LF_TRY(fp_fft_two_pass<O>(c, wi, 20, n1, (const elt_t*)mid, n2, row, 1, (long long)n1));
  }
  return LFGPU_OK;
}

extern "C" int lfgpu_fp128_fft(lfgpu_ctx* c, int dir, size_t rows, size_t n, const uint64_t omega[2], uint64_t omega_order, void* d_A,
                               size_t ld) {
  return fft_any<Fp128Ops>(c, "fp128_fft", dir, rows, n, omega, omega_order, d_A, ld);
}
// FFT<Fp2<Fp<1>>>::fftb / fftf over p = 2^64 - 2^32 + 1 (fft_test.cc:205-229).  omega = {re, im}; the usual root is real.
extern "C" int lfgpu_f64_2_fft(lfgpu_ctx* c, int dir, size_t rows, size_t n, const uint64_t omega[2], uint64_t omega_order, void* d_A,
                               size_t ld) {
  if (omega && (omega[0] >= F64_P || omega[1] >= F64_P)) return lf_fail(c, LFGPU_ERR_ARG, "f64_2_fft: omega is not reduced");
  if (omega && omega[1] == 0) return fft_any<F64x2Ops<true>>(c, "f64_2_fft", dir, rows, n, omega, omega_order, d_A, ld);
  return fft_any<F64x2Ops<false>>(c, "f64_2_fft", dir, rows, n, omega, omega_order, d_A, ld);
}

// Build (and cache) LCH14 twiddle tables for one tile pass.
//   with_coset: fold `coset` into tbl (pass A / single pass); otherwise tbl is coset-free
//   and base[ii*nb + blk] = twiddle(i, coset ^ (blk << logT)) carries coset and block bits.
static int lch_tables(lfgpu_ctx* c, const GfHostCtx* g, u32 i_lo, u32 logT, u64 coset, bool with_coset, u32 nb,
                      LchTables* out) {
  std::string key = keyf("lch:%u:%u:%u:%llx:%d:%u", g->k, i_lo, logT, (u64)coset, (int)with_coset, nb);
  void *dt = nullptr, *db = nullptr;
  u32 off = 0;
  for (u32 ii = 0; ii < logT; ++ii) {
    out->off[ii] = off;
    off += 1u << (logT - 1 - ii);
  }
  if (!lf_table_lookup(c, key, &dt)) {
    std::vector<elt_t> tbl(off ? off : 1);
    for (u32 ii = 0; ii < logT; ++ii) {
      u32 i = i_lo + ii, cnt = 1u << (logT - 1 - ii);
      for (u32 u = 0; u < cnt; ++u) {
        u64 x = (u64)u << (i + 1);
        if (with_coset) x ^= coset;
        tbl[out->off[ii] + u] = h_lch14_twiddle(g, i, x);
      }
    }
    LF_TRY(lf_table(c, key, tbl.data(), tbl.size() * 16, &dt));
  }
  out->tbl = (const elt_t*)dt;
  out->base = nullptr;
  out->nb = nb;
  if (!with_coset) {
    std::string kb = key + ":base";
    if (!lf_table_lookup(c, kb, &db)) {
      std::vector<elt_t> base((size_t)logT * nb);
      for (u32 ii = 0; ii < logT; ++ii)
        for (u32 b = 0; b < nb; ++b)
          base[(size_t)ii * nb + b] = h_lch14_twiddle(g, i_lo + ii, coset ^ ((u64)b << (i_lo + logT)));
      LF_TRY(lf_table(c, kb, base.data(), base.size() * 16, &db));
    }
    out->base = (const elt_t*)db;
  }
  return LFGPU_OK;
}

extern "C" int lfgpu_gf2128_lch14_fft(lfgpu_ctx* c, int k, int dir, size_t rows, unsigned l, uint64_t coset,
                                      void* d_B, size_t ld) {
  if (!c || (!d_B && rows)) return lf_fail(c, LFGPU_ERR_ARG, "lch14_fft: null argument");
  const GfHostCtx* g = lf_gf_ctx(c, k);
  if (!g) return lf_fail(c, LFGPU_ERR_ARG, "lch14_fft: subfield_log_bits must be 4 or 5");
  if (l > g->sub_bits) return lf_fail(c, LFGPU_ERR_ARG, "lch14_fft: l <= kSubFieldBits violated (lch14.h:107)");
  if (rows == 0 || l == 0) return LFGPU_OK;
  // the two-pass tile plan splits l = (l - 10) + 10 with a first tile of at most 2^tile_log points: l <= 22; batches of
  // >= 32 rows take the bit-sliced path, whose passes are generic in l (bounded here by its u32 column indices and the
  // 2^l x 128-byte internal buffer per 32 rows)
  if (l > (rows >= 32 ? 24u : 10u + (unsigned)c->tile_log)) return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "lch14_fft: l = %u too large for %zu rows", l, rows);
  if (ld < ((size_t)1 << l)) return lf_fail(c, LFGPU_ERR_ARG, "lch14_fft: ld < 2^l");
  if (rows > 0x7fffffffu) return lf_fail(c, LFGPU_ERR_ARG, "lch14_fft: too many rows");
  LF_HIP(c, hipSetDevice(c->device));
  LF_TRY(set_lds_limit(c));
  const int inverse = dir ? 1 : 0;
  {  // batches of >= 32 rows take the bit-sliced tower path (lch_bs.hip); LFGPU_LCH_BS=0 disables it
    static int bs = -1;
    if (bs < 0) {
      const char* e = getenv("LFGPU_LCH_BS");
      bs = (e && atoi(e) == 0) ? 0 : 1;
    }
    if (bs && rows >= 32 && l >= 7) return lf_lch14_fft_bitsliced(c, k, inverse, rows, l, coset, d_B, ld);
  }
  if (l <= (unsigned)c->tile_log) {
    TilePlan p = plan_single(c, d_B, rows, l, ld);
    LchTables t{};
    LF_TRY(lch_tables(c, g, 0, l, coset, true, 1, &t));
    u32 ntiles = (u32)((rows + (1u << p.logC) - 1) >> p.logC);
    size_t lds = ((size_t)16 << p.logT) << p.logC;
    launch_lch(c, dim3(ntiles, 1), lds, p, inverse, t);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  const u32 lo = 10, logn1 = l - lo;
  const size_t n1 = (size_t)1 << logn1, n2 = (size_t)1 << lo;
  TilePlan pa{}, pb{};
  LchTables ta{}, tb{};
  // pass A: stages i >= lo over k1 (stride n2); twiddle index u = k1 >> (ii+1): no block term
  pa.logT = logn1;
  pa.logC = (u32)c->tile_log - logn1;
  if (pa.logC > lo) pa.logC = lo;
  pa.src = (const elt_t*)d_B;
  pa.dst = (elt_t*)d_B;
  pa.src_row = pa.dst_row = (long long)ld;
  pa.src_tile = pa.dst_tile = 1ll << pa.logC;
  pa.sk = pa.dk = (long long)n2;
  pa.sc = pa.dc = 1;
  pa.nbatch = (u32)n2;
  pa.kfast_src = pa.kfast_dst = 0;
  LF_TRY(lch_tables(c, g, lo, logn1, coset, true, 1, &ta));
  // pass B: stages i < lo on contiguous blocks k1; C consecutive blocks per tile
  pb.logT = lo;
  pb.logC = (u32)c->tile_log - lo;
  if (pb.logC > logn1) pb.logC = logn1;
  pb.src = (const elt_t*)d_B;
  pb.dst = (elt_t*)d_B;
  pb.src_row = pb.dst_row = (long long)ld;
  pb.src_tile = pb.dst_tile = (long long)n2 << pb.logC;
  pb.sk = pb.dk = 1;
  pb.sc = pb.dc = (long long)n2;
  pb.nbatch = (u32)n1;
  pb.kfast_src = pb.kfast_dst = 1;
  LF_TRY(lch_tables(c, g, 0, lo, coset, false, (u32)n1, &tb));
  size_t lds_a = ((size_t)16 << pa.logT) << pa.logC, lds_b = ((size_t)16 << pb.logT) << pb.logC;
  dim3 ga((u32)(n2 >> pa.logC), (u32)rows), gb((u32)(n1 >> pb.logC), (u32)rows);
  if (!inverse) {  // FFT: stages l-1 .. 0
    launch_lch(c, ga, lds_a, pa, 0, ta);
    launch_lch(c, gb, lds_b, pb, 0, tb);
  } else {  // IFFT: stages 0 .. l-1
    launch_lch(c, gb, lds_b, pb, 1, tb);
    launch_lch(c, ga, lds_a, pa, 1, ta);
  }
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}

extern "C" int lfgpu_fp128_fft_host(lfgpu_ctx* c, int dir, size_t n, const uint64_t omega[2], uint64_t omega_order,
                                    void* h_A) {
  if (!c || !h_A) return LFGPU_ERR_ARG;
  void* d = nullptr;
  LF_TRY(lf_scratch2(c, n * 16, &d));
  LF_HIP(c, hipMemcpyAsync(d, h_A, n * 16, hipMemcpyHostToDevice, c->stream));
  LF_TRY(lfgpu_fp128_fft(c, dir, 1, n, omega, omega_order, d, n));
  LF_HIP(c, hipMemcpyAsync(h_A, d, n * 16, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipStreamSynchronize(c->stream));
  return LFGPU_OK;
}

extern "C" int lfgpu_f64_2_fft_host(lfgpu_ctx* c, int dir, size_t n, const uint64_t omega[2], uint64_t omega_order, void* h_A) {
  if (!c || !h_A) return LFGPU_ERR_ARG;
  void* d = nullptr;
  LF_TRY(lf_scratch2(c, n * 16, &d));
  LF_HIP(c, hipMemcpyAsync(d, h_A, n * 16, hipMemcpyHostToDevice, c->stream));
  LF_TRY(lfgpu_f64_2_fft(c, dir, 1, n, omega, omega_order, d, n));
  LF_HIP(c, hipMemcpyAsync(h_A, d, n * 16, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipStreamSynchronize(c->stream));
  return LFGPU_OK;
}

extern "C" int lfgpu_gf2128_lch14_fft_host(lfgpu_ctx* c, int k, int dir, unsigned l, uint64_t coset, void* h_B) {
  if (!c || !h_B) return LFGPU_ERR_ARG;
  size_t n = (size_t)1 << l;
  void* d = nullptr;
  LF_TRY(lf_scratch2(c, n * 16, &d));
  LF_HIP(c, hipMemcpyAsync(d, h_B, n * 16, hipMemcpyHostToDevice, c->stream));
  LF_TRY(lfgpu_gf2128_lch14_fft(c, k, dir, 1, l, coset, d, n));
  LF_HIP(c, hipMemcpyAsync(h_B, d, n * 16, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipStreamSynchronize(c->stream));
  return LFGPU_OK;
}
