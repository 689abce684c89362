// fp_tile_arith.h -- the Fp128 add, sub and twiddle product of K1's 1024 x 4 tile kernels (csrc/fft.hip).
//
// Same values as fp_add / fp_sub / fp_mul of fields.h for canonical inputs (< p), with fewer VALU instructions:
//   - fpt_mul: the first carry of every product column is written into the high half of the next column's accumulator
//     instead of added to a zeroed one (one v_mov per column instead of two); the REDC never forms m = -U: it computes
//     T_hi - U + (U >> 20) + cy and adds p when that is negative (a sign from two carry masks merged by one SALU
//     instruction): 27 -> 19 VALU instructions for the REDC, 71 -> 63 -> 55 per product; the first mad of columns 3, 4 and
//     5 (a_i b3) cannot carry for w < p and has no capture: 52; nor can column 2's (a0 b2), for any a and w, and column 1's
//     first mad reads {acc0.hi, 0} as its addend and writes a fresh pair, which spares column 0 its 64-bit move: 50.
//   - fpt_add: the carry-out of a + b stays a lane mask and is merged with the borrow of (a + b) - p by one SALU
//     instruction: 14 -> 12 VALU instructions.
//   - fpt_sub: the borrow of a - b, kept in an SGPR pair, is the carry-in of the + p chain: 10 -> 9.
// With these three every value stays canonical, so what the tiles keep in LDS and write to HBM is unchanged.
//
// The pair fp_fft_tile_1024x4_tws also lets a butterfly's u side be *lazy*: any 128-bit value congruent to the element, not
// necessarily < p.  In x = u + w v, y = u - w v the product w v is canonical whatever v was (see fpt_mul), so
//   - fpt_add_lazy(u, t), u lazy, t < p: u + t < 2^128 + p, one fold under the carry mask, 9 instructions instead of 12;
//   - fpt_sub(u, t) as it is: u - t in (-p, 2^128), + p on borrow;
//   - fpt_canon(u): lazy -> canonical, 8 instructions, where a value leaves the scheme (what pass B stores).
//
// Wait states: gfx950 needs 2 between a VALU that writes an SGPR or VCC and a VALU that reads it (carry-in, mask), and
// hipcc inserts none inside an asm statement, so every such link carries an `s_nop 1`, as in fields.h.  The same is kept
// in front of the SALU instructions that read a mask a VALU wrote.  Each asm statement keeps VCC and its SGPR masks live
// only inside itself, and the ones with SALU instructions clobber SCC: the compiler may hold a live SCC across them (the carry
// of a 64-bit address add, a loop's branch condition).
#pragma once
#include "fields.h"

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ elt_t fpt_add(elt_t a, elt_t b) {
  FP_W(a, a0, a1, a2, a3);
  FP_W(b, b0, b1, b2, b3);
  u32 s0, s1, s2, s3, d0, d1, d2, d3;
  u64 c;
  asm("v_add_co_u32 %0, vcc, %9, %13\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %1, vcc, %10, %14, vcc\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %2, vcc, %11, %15, vcc\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %3, %8, %12, %16, vcc\n\t"  // carry-out of a + b: lane mask c
      // s - p, p = {1, 0, 0, 0xfffff000}; final borrow set <=> s < p
      "v_subrev_co_u32 %4, vcc, 1, %0\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %5, vcc, 0, %1, vcc\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %6, vcc, 0, %2, vcc\n\t"
      "s_nop 1\n\t"
      "v_subb_co_u32 %7, vcc, %3, %17, vcc\n\t"
      "s_nop 1\n\t"
      "s_andn2_b64 vcc, vcc, %8\n\t"  // keep s <=> (c:s) < p <=> borrow and no carry
      "v_cndmask_b32 %4, %4, %0, vcc\n\t"
      "v_cndmask_b32 %5, %5, %1, vcc\n\t"
      "v_cndmask_b32 %6, %6, %2, vcc\n\t"
      "v_cndmask_b32 %7, %7, %3, vcc"
      : "=&v"(s0), "=&v"(s1), "=&v"(s2), "=&v"(s3), "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3), "=&s"(c)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(b0), "v"(b1), "v"(b2), "v"(b3), "v"(0xfffff000u)
      : "vcc", "scc");
  return FP_PACK(d0, d1, d2, d3);
}

// a + b for a lazy (any 128-bit value), b < p; the result is lazy.  s = a + b < 2^128 + p: if the 128-bit add carries, s - p lies
// in [2^108 - 1, 2^128) and is s_low - p mod 2^128 (s_low < p then, so that subtraction borrows: the two 2^128 cancel); otherwise
// s_low is the result.  - p under the carry mask c: - c at limb 0 (the mask is the borrow-in), - 0xfffff000 at limb 3, the mirror
// image of fpt_sub's + p.  No SALU instruction, so SCC is left alone.
__device__ __forceinline__ elt_t fpt_add_lazy(elt_t a, elt_t b) {
  FP_W(a, a0, a1, a2, a3);
  FP_W(b, b0, b1, b2, b3);
  u32 d0, d1, d2, d3, e3;
  u64 c;
  asm("v_add_co_u32 %0, vcc, %6, %10\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %1, vcc, %7, %11, vcc\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %2, vcc, %8, %12, vcc\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %3, %5, %9, %13, vcc\n\t"  // carry-out of a + b: lane mask c
      "s_nop 1\n\t"
      "v_cndmask_b32 %4, 0, %14, %5\n\t"
      "v_subbrev_co_u32 %0, vcc, 0, %0, %5\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %1, vcc, 0, %1, vcc\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %2, vcc, 0, %2, vcc\n\t"
      "s_nop 1\n\t"
      "v_subb_co_u32 %3, vcc, %3, %4, vcc"
      : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3), "=&v"(e3), "=&s"(c)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(b0), "v"(b1), "v"(b2), "v"(b3), "v"(0xfffff000u)
      : "vcc");
  return FP_PACK(d0, d1, d2, d3);
}

// a lazy -> the canonical value: a - p if that does not borrow (a >= p; a < 2^128 < 2p, so once is enough), else a
__device__ __forceinline__ elt_t fpt_canon(elt_t a) {
  FP_W(a, a0, a1, a2, a3);
  u32 d0, d1, d2, d3;
  asm("v_subrev_co_u32 %0, vcc, 1, %4\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %1, vcc, 0, %5, vcc\n\t"
      "s_nop 1\n\t"
      "v_subbrev_co_u32 %2, vcc, 0, %6, vcc\n\t"
      "s_nop 1\n\t"
      "v_subb_co_u32 %3, vcc, %7, %8, vcc\n\t"  // borrow <=> a < p: keep a
      "s_nop 1\n\t"
      "v_cndmask_b32 %0, %0, %4, vcc\n\t"
      "v_cndmask_b32 %1, %1, %5, vcc\n\t"
      "v_cndmask_b32 %2, %2, %6, vcc\n\t"
      "v_cndmask_b32 %3, %3, %7, vcc"
      : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(0xfffff000u)
      : "vcc");
  return FP_PACK(d0, d1, d2, d3);
}

// a - b for a < p or a lazy, b < p.  With a < p the result is canonical; with a lazy, d = a - b lies in (-p, 2^128): a borrow
// means d < 0 and d + p in (0, p), no borrow leaves d in [0, 2^128), so the result is lazy: this is the lazy subtraction as well.
__device__ __forceinline__ elt_t fpt_sub(elt_t a, elt_t b) {
  FP_W(a, a0, a1, a2, a3);
  FP_W(b, b0, b1, b2, b3);
  u32 d0, d1, d2, d3, e3;
  u64 bw;
  asm("v_sub_co_u32 %0, vcc, %6, %10\n\t"
      "s_nop 1\n\t"
      "v_subb_co_u32 %1, vcc, %7, %11, vcc\n\t"
      "s_nop 1\n\t"
      "v_subb_co_u32 %2, vcc, %8, %12, vcc\n\t"
      "s_nop 1\n\t"
      "v_subb_co_u32 %3, %5, %9, %13, vcc\n\t"  // borrow of a - b: lane mask bw
      "s_nop 1\n\t"
      // borrow => + p: + bw at limb 0 (the mask is the carry-in), + 0xfffff000 at limb 3
      "v_cndmask_b32 %4, 0, %14, %5\n\t"
      "v_addc_co_u32 %0, vcc, 0, %0, %5\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %2, vcc, 0, %2, vcc\n\t"
      "s_nop 1\n\t"
      "v_addc_co_u32 %3, vcc, %4, %3, vcc"
      : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3), "=&v"(e3), "=&s"(bw)
      : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(b0), "v"(b1), "v"(b2), "v"(b3), "v"(0xfffff000u)
      : "vcc");
  return FP_PACK(d0, d1, d2, d3);
}

// acc(64) += x*y, y a limb of the twiddle under the constraint C: "v", or "s" for a wave-uniform twiddle held in SGPRs (the one
// scalar source a VOP3 instruction may read; everything else of the product stays in VGPRs).  FPT_MADW WRITES the carry-out to
// ov (the first carry of a column: ov would be 0), FPT_MADC adds it, FPT_MAD has none to catch.
#define FPT_MAD(C, acc, x, y) asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(x), C(y) : "vcc")
#define FPT_MADC(C, acc, ov, x, y) \
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\ts_nop 1\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc" : "+v"(acc), "+v"(ov) : "v"(x), C(y) : "vcc")
#define FPT_MADW(C, acc, ov, x, y) \
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\ts_nop 1\n\tv_addc_co_u32 %1, vcc, 0, 0, vcc" : "+v"(acc), "=v"(ov) : "v"(x), C(y) : "vcc")
#define FPT_COL(tk, acc, ov) \
  tk = (u32)(acc);           \
  acc = ((acc) >> 32) | ((u64)(ov) << 32)
// T = a w in product scanning, t0..t7, for the twiddle's limbs under C.  Column 1's first mad is out of place, its addend
// {acc0.hi, 0} (< 2^64: (2^32 - 1)^2 + 2^32 - 1).  The bare FPT_MADs cannot carry: a0 b2 for every a and w, a0 b3, a1 b3 and
// a2 b3 for b3 <= 0xfffff000 (see fpt_mul).
#define FPT_COLUMNS(C)                                                                                 \
  asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(acc0) : "v"(a0), C(b0) : "vcc");                       \
  t0 = (u32)acc0;                                                                                      \
  asm("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=v"(acc) : "v"(a0), C(b1), "v"(acc0 >> 32) : "vcc");      \
  FPT_MADW(C, acc, ov, a1, b0);                                                                        \
  FPT_COL(t1, acc, ov);                                                                                \
  FPT_MAD(C, acc, a0, b2);                                                                             \
  FPT_MADW(C, acc, ov, a1, b1);                                                                        \
  FPT_MADC(C, acc, ov, a2, b0);                                                                        \
  FPT_COL(t2, acc, ov);                                                                                \
  FPT_MAD(C, acc, a0, b3);                                                                             \
  FPT_MADW(C, acc, ov, a1, b2);                                                                        \
  FPT_MADC(C, acc, ov, a2, b1);                                                                        \
  FPT_MADC(C, acc, ov, a3, b0);                                                                        \
  FPT_COL(t3, acc, ov);                                                                                \
  FPT_MAD(C, acc, a1, b3);                                                                             \
  FPT_MADW(C, acc, ov, a2, b2);                                                                        \
  FPT_MADC(C, acc, ov, a3, b1);                                                                        \
  FPT_COL(t4, acc, ov);                                                                                \
  FPT_MAD(C, acc, a2, b3);                                                                             \
  FPT_MADW(C, acc, ov, a3, b2);                                                                        \
  FPT_COL(t5, acc, ov);                                                                                \
  FPT_MAD(C, acc, a3, b3);                                                                             \
  t6 = (u32)acc;                                                                                       \
  t7 = (u32)(acc >> 32)

// a * w / 2^128 mod p (Montgomery), as fp_mul for a, w < p.  a may be any 128-bit value (lazy) as long as w < p: T = a w < 2^128 p,
// so T_hi < p, (T + m p) / 2^128 < 2p and W in [-p, p) as below, and the result is canonical.  Product scanning with 16 v_mad_u64_u32; the carries of column k
// go to ov, which becomes the high half of column k + 1's accumulator {acc.hi, ov}.
//
// PRECONDITION: the SECOND argument is < p (a twiddle; T4Ops<Fp128Ops>::mul_tw in fft.hip passes nothing else).  Besides the
// range of the REDC, three carry captures rest on it.  p = 2^128 - 2^108 + 1, so the top limb of w < p is b3 <= 0xfffff000.
// Columns 3, 4 and 5 start with a0 b3, a1 b3 and a2 b3.  The accumulator that enters such a column is {acc.hi, ov} with
// acc.hi < 2^32 and ov <= 3 (at most three captures in the column before), so it is < 2^34; the first product is at most
// (2^32 - 1) 0xfffff000 = 2^64 - 2^44 - 2^32 + 2^12; the sum is < 2^64 - 2^44 + 2^34 < 2^64 whatever a is, lazy values
// included.  That mad cannot carry and is a bare FP_MAD; the column's second mad is the one whose capture writes ov.  13 -> 10
// captures, 55 -> 52 VALU instructions per product, same values.  With b3 = 0xffffffff (no field element) column 3's first mad
// does wrap: tests/test_fp_tile_mul_carries.py has the model, the case and the inputs that reach these carries on the device.
//
// Column 2 starts with a0 b2, which that bound does not cover (b2 may be 0xffffffff), but another does, for every a and w: column
// 1's true sum is at most (2^32 - 2) + 2 (2^32 - 1)^2 = 2^65 - 3 2^32, so column 2's accumulator comes in at no more than
// 2^33 - 3, and a0 b2 <= 2^64 - 2^33 + 1 brings it to 2^64 - 2 at the most.  Its capture is gone too and a1 b1's writes ov: 9
// captures.  Column 0 has no carry, so column 1's accumulator is {acc0.hi, 0}; its first mad takes that pair as the addend
// of an out-of-place v_mad_u64_u32 (the pair's high half is a register the compiler keeps at zero, its low half one v_mov_b32)
// instead of shifting acc0 in place, which cost a v_mov_b32 and a v_mov_b64.  52 -> 50 (tests/test_fp_tile_mul50.py).
//
// SW: the twiddle is wave-uniform and its limbs are SGPR operands of the mads (fpt_mul_sw; the stage twiddles of a round whose
// twiddle index is the same in every lane of a wave, fetched by scalar loads).  A value that is not uniform must not come here:
// the compiler would take its first active lane's.  Same schedule, same values.
template <bool SW>
__device__ __forceinline__ elt_t fpt_mul_t(elt_t a, elt_t b) {
  FP_W(a, a0, a1, a2, a3);
  FP_W(b, b0, b1, b2, b3);
  u32 t0, t1, t2, t3, t4, t5, t6, t7, ov;
  u64 acc0, acc;
  if constexpr (SW) {
    FPT_COLUMNS("s");
  } else {
    FPT_COLUMNS("v");
  }
  // REDC in one 128-bit step, with U = (t0, t1, t2, u3), u3 = t3 + k, k = t0 << 12 (mod 2^32), cy = carry of t3 + k.
  // fp_mul computes m = -U and (T + m p) / 2^128 = T_hi + m - (m >> 20) + delta, delta = carry-out of T_lo + m, which is
  // cy | ([k = 0] & [U != 0]).  For U != 0, m >> 20 = 2^108 - ceil(U / 2^20) with ceil(U / 2^20) = (U >> 20) + [k != 0]
  // (U and t0 share their low 20 bits), and m - 2^108 = p - 1 - U; a carry implies k != 0, so the small terms sum to cy:
  //   W = T_hi - U + (U >> 20) + cy = (T + m p) / 2^128 - p,   -p <= W < p,   result W, or W + p if W < 0.
  // U = 0 gives k = cy = 0 and W = T_hi < p, as fp_mul.  The sign: with b = borrow-out of T_hi - U and c = carry-out of
  // + (U >> 20) + cy, W = (d3..d0) + (c - b) 2^128, so W < 0 <=> b and no c.  The cy link needs no s_nop: eight VALU
  // instructions lie between its write and its read.  d0..d3 are outputs of their own, not T_hi's registers, so the
  // allocator can put the result where its user wants it (tied to T_hi, pass A's one-tile kernel needed 23 more VALU).
  // U and U >> 20 have none: u3 is formed in t3's register, and once T_hi - U has read U the shifts overwrite it (t0..t3
  // are dead after the reduction).  Five temporaries fewer, which keeps pass A at 71 VGPRs with the 50-instruction product.
  const u32 k = t0 << 12;
  u32 d0, d1, d2, d3;
  {
    u32 e3;
    u64 cy, b;
    asm("v_add_co_u32 %7, %9, %7, %11\n\t"  // u3 (in t3's register), cy
        "v_sub_co_u32 %0, vcc, %13, %4\n\t"  // T_hi - U
        "s_nop 1\n\t"
        "v_subb_co_u32 %1, vcc, %14, %5, vcc\n\t"
        "s_nop 1\n\t"
        "v_subb_co_u32 %2, vcc, %15, %6, vcc\n\t"
        "s_nop 1\n\t"
        "v_subb_co_u32 %3, %10, %16, %7, vcc\n\t"  // borrow-out: lane mask b
        "v_alignbit_b32 %4, %5, %4, 20\n\t"  // U >> 20, in U's registers
        "v_alignbit_b32 %5, %6, %5, 20\n\t"
        "v_alignbit_b32 %6, %7, %6, 20\n\t"
        "v_lshrrev_b32 %7, 20, %7\n\t"
        "v_addc_co_u32 %0, vcc, %0, %4, %9\n\t"  // + (U >> 20) + cy, cy the carry-in
        "s_nop 1\n\t"
        "v_addc_co_u32 %1, vcc, %1, %5, vcc\n\t"
        "s_nop 1\n\t"
        "v_addc_co_u32 %2, vcc, %2, %6, vcc\n\t"
        "s_nop 1\n\t"
        "v_addc_co_u32 %3, %9, %3, %7, vcc\n\t"  // carry-out: lane mask c (in cy's SGPR pair)
        "s_nop 1\n\t"
        "s_andn2_b64 %9, %10, %9\n\t"  // W < 0 <=> b and no c
        // W < 0 => + p: + 1 at limb 0 (the mask is the carry-in), + 0xfffff000 at limb 3, as fpt_sub
        "v_cndmask_b32 %8, 0, %12, %9\n\t"
        "v_addc_co_u32 %0, vcc, 0, %0, %9\n\t"
        "s_nop 1\n\t"
        "v_addc_co_u32 %1, vcc, 0, %1, vcc\n\t"
        "s_nop 1\n\t"
        "v_addc_co_u32 %2, vcc, 0, %2, vcc\n\t"
        "s_nop 1\n\t"
        "v_addc_co_u32 %3, vcc, %8, %3, vcc"
        : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3), "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3), "=&v"(e3), "=&s"(cy), "=&s"(b)
        : "v"(k), "v"(0xfffff000u), "v"(t4), "v"(t5), "v"(t6), "v"(t7)
        : "vcc", "scc");
    // t0..t3 hold U >> 20 from here on, not the column words: do not read them behind the reduction
  }
  return FP_PACK(d0, d1, d2, d3);
}
__device__ __forceinline__ elt_t fpt_mul(elt_t a, elt_t b) { return fpt_mul_t<false>(a, b); }
__device__ __forceinline__ elt_t fpt_mul_sw(elt_t a, elt_t b) { return fpt_mul_t<true>(a, b); }
#else
// the host pass of a kernel that calls them, and host code: the portable forms (same values)
LF_HD elt_t fpt_add(elt_t a, elt_t b) { return fp_add_c(a, b); }
LF_HD elt_t fpt_sub(elt_t a, elt_t b) { return fp_sub_c(a, b); }
LF_HD elt_t fpt_canon(elt_t a) { return fp_canon128(a); }
LF_HD elt_t fpt_add_lazy(elt_t a, elt_t b) {  // the fold of the carry: 2^128 = p + (2^128 - p)
  const u64 lo = a.lo + b.lo, c0 = lo < a.lo, h0 = a.hi + b.hi, hi = h0 + c0;
  if (!((h0 < a.hi) | (hi < c0))) return elt_t{lo, hi};
  return elt_t{lo - FP_P_LO, hi - FP_P_HI - (lo < FP_P_LO)};
}
LF_HD elt_t fpt_mul(elt_t a, elt_t b) { return fp_mul_c(fp_canon128(a), b); }
LF_HD elt_t fpt_mul_sw(elt_t a, elt_t b) { return fpt_mul(a, b); }
#endif
