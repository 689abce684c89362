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
//
// The default pair at n = 2^20 (fp_fft_tile_1024x4_lean, and fp_fft_tile_1024x4_tw2<T4Ilp<Fp128Ops>, ..> before it) issues the
// same arithmetic two operations at a time: fpt_mul2_t, fpt_bfly2_lazy, fpt_bfly_lazy and fpt_canon2 at the end of this file
// fill those wait states with the other operation's instructions, and fpt_bfly2_full does the same for two butterflies with
// full sums (fp_fft_tile_1024x4_lean only).  Same values, same VALU instructions; the single routines above serve every other kernel.
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

// ------------------------------------------------------------------ the paired routines (fp_fft_tile_1024x4_ilp)
// The same values as the routines above, two independent operations per call, issued so that a carry's consumer stands behind
// its producer by independent VALU instructions of the other operation instead of an `s_nop 1`: each chain keeps its carry in a
// register of its own, VCC or an SGPR pair (the VOP3 forms take any pair as carry-in and carry-out).  The rule is the one above,
// 2 wait states between a VALU write of VCC or an SGPR pair and a VALU read of it; every instruction in between counts one, and
// where only one lies in between an `s_nop 0` supplies the other.  tests/test_fp128_tile_ilp.py checks the rule on the built code.

// Two butterflies: (x, y) = (u + t lazy, u - t) for (u, t) = (xp, yp) and (xq, yq), t < p.  Four chains of fpt_add_lazy / fpt_sub,
// limb by limb: u + t of p in VCC, u - t of p in c1, q's in c2 and c3, three instructions between every link.  y's limbs take t's
// registers (u_i + t_i is read first).  36 VALU instructions, no s_nop.
__device__ __forceinline__ void fpt_bfly2_lazy(elt_t& xp, elt_t& yp, elt_t& xq, elt_t& yq) {
  FP_W(xp, up0, up1, up2, up3);
  FP_W(yp, tp0, tp1, tp2, tp3);
  FP_W(xq, uq0, uq1, uq2, uq3);
  FP_W(yq, tq0, tq1, tq2, tq3);
  u32 dp0, dp1, dp2, dp3, dq0, dq1, dq2, dq3, eap, esp, eaq, esq;
  u64 c1, c2, c3;
  asm("v_add_co_u32 %[dp0], vcc, %[up0], %[tp0]\n\t"
      "v_sub_co_u32 %[tp0], %[c1], %[up0], %[tp0]\n\t"
      "v_add_co_u32 %[dq0], %[c2], %[uq0], %[tq0]\n\t"
      "v_sub_co_u32 %[tq0], %[c3], %[uq0], %[tq0]\n\t"
      "v_addc_co_u32 %[dp1], vcc, %[up1], %[tp1], vcc\n\t"
      "v_subb_co_u32 %[tp1], %[c1], %[up1], %[tp1], %[c1]\n\t"
      "v_addc_co_u32 %[dq1], %[c2], %[uq1], %[tq1], %[c2]\n\t"
      "v_subb_co_u32 %[tq1], %[c3], %[uq1], %[tq1], %[c3]\n\t"
      "v_addc_co_u32 %[dp2], vcc, %[up2], %[tp2], vcc\n\t"
      "v_subb_co_u32 %[tp2], %[c1], %[up2], %[tp2], %[c1]\n\t"
      "v_addc_co_u32 %[dq2], %[c2], %[uq2], %[tq2], %[c2]\n\t"
      "v_subb_co_u32 %[tq2], %[c3], %[uq2], %[tq2], %[c3]\n\t"
      "v_addc_co_u32 %[dp3], vcc, %[up3], %[tp3], vcc\n\t"  // the carries and borrows out: lane masks
      "v_subb_co_u32 %[tp3], %[c1], %[up3], %[tp3], %[c1]\n\t"
      "v_addc_co_u32 %[dq3], %[c2], %[uq3], %[tq3], %[c2]\n\t"
      "v_subb_co_u32 %[tq3], %[c3], %[uq3], %[tq3], %[c3]\n\t"
      // carry => - p, borrow => + p: -+ the mask at limb 0 (it is the borrow- or carry-in), -+ 0xfffff000 at limb 3
      "v_cndmask_b32 %[eap], 0, %[k], vcc\n\t"
      "v_cndmask_b32 %[esp], 0, %[k], %[c1]\n\t"
      "v_cndmask_b32 %[eaq], 0, %[k], %[c2]\n\t"
      "v_cndmask_b32 %[esq], 0, %[k], %[c3]\n\t"
      "v_subbrev_co_u32 %[dp0], vcc, 0, %[dp0], vcc\n\t"
      "v_addc_co_u32 %[tp0], %[c1], 0, %[tp0], %[c1]\n\t"
      "v_subbrev_co_u32 %[dq0], %[c2], 0, %[dq0], %[c2]\n\t"
      "v_addc_co_u32 %[tq0], %[c3], 0, %[tq0], %[c3]\n\t"
      "v_subbrev_co_u32 %[dp1], vcc, 0, %[dp1], vcc\n\t"
      "v_addc_co_u32 %[tp1], %[c1], 0, %[tp1], %[c1]\n\t"
      "v_subbrev_co_u32 %[dq1], %[c2], 0, %[dq1], %[c2]\n\t"
      "v_addc_co_u32 %[tq1], %[c3], 0, %[tq1], %[c3]\n\t"
      "v_subbrev_co_u32 %[dp2], vcc, 0, %[dp2], vcc\n\t"
      "v_addc_co_u32 %[tp2], %[c1], 0, %[tp2], %[c1]\n\t"
      "v_subbrev_co_u32 %[dq2], %[c2], 0, %[dq2], %[c2]\n\t"
      "v_addc_co_u32 %[tq2], %[c3], 0, %[tq2], %[c3]\n\t"
      "v_subb_co_u32 %[dp3], vcc, %[dp3], %[eap], vcc\n\t"
      "v_addc_co_u32 %[tp3], %[c1], %[esp], %[tp3], %[c1]\n\t"
      "v_subb_co_u32 %[dq3], %[c2], %[dq3], %[eaq], %[c2]\n\t"
      "v_addc_co_u32 %[tq3], %[c3], %[esq], %[tq3], %[c3]"
      : [dp0] "=&v"(dp0), [dp1] "=&v"(dp1), [dp2] "=&v"(dp2), [dp3] "=&v"(dp3), [dq0] "=&v"(dq0), [dq1] "=&v"(dq1), [dq2] "=&v"(dq2),
        [dq3] "=&v"(dq3), [tp0] "+v"(tp0), [tp1] "+v"(tp1), [tp2] "+v"(tp2), [tp3] "+v"(tp3), [tq0] "+v"(tq0), [tq1] "+v"(tq1),
        [tq2] "+v"(tq2), [tq3] "+v"(tq3), [eap] "=&v"(eap), [esp] "=&v"(esp), [eaq] "=&v"(eaq), [esq] "=&v"(esq), [c1] "=&s"(c1),
        [c2] "=&s"(c2), [c3] "=&s"(c3)
      : [up0] "v"(up0), [up1] "v"(up1), [up2] "v"(up2), [up3] "v"(up3), [uq0] "v"(uq0), [uq1] "v"(uq1), [uq2] "v"(uq2), [uq3] "v"(uq3),
        [k] "v"(0xfffff000u)
      : "vcc");
  xp = FP_PACK(dp0, dp1, dp2, dp3);
  yp = FP_PACK(tp0, tp1, tp2, tp3);
  xq = FP_PACK(dq0, dq1, dq2, dq3);
  yq = FP_PACK(tq0, tq1, tq2, tq3);
}

// Two butterflies with full sums: (x, y) = (u + t, u - t) canonical for (u, t) = (xp, yp) and (xq, yq), all four < p: fpt_add and
// fpt_sub twice, interleaved like fpt_bfly2_lazy.  Six chains: the sums s = u + t (carry-out kept in ap / aq until the end), the
// differences u - t (borrow in sp / sq, which then carries the + p chain, as in fpt_sub), and s - p (borrow in VCC / bq).  Every
// link has at least two VALU instructions of other chains between its write and its read, the two s_andn2_b64 (keep s <=> borrow
// and no carry, as fpt_add) stand two VALU instructions behind the last write of their masks, and the v_cndmask that follow read
// a mask an SALU instruction wrote.  y's limbs take t's registers.  42 VALU instructions, the same as two fpt_add and two
// fpt_sub, no s_nop.
__device__ __forceinline__ void fpt_bfly2_full(elt_t& xp, elt_t& yp, elt_t& xq, elt_t& yq) {
  FP_W(xp, up0, up1, up2, up3);
  FP_W(yp, tp0, tp1, tp2, tp3);
  FP_W(xq, uq0, uq1, uq2, uq3);
  FP_W(yq, tq0, tq1, tq2, tq3);
  u32 sp0, sp1, sp2, sp3, sq0, sq1, sq2, sq3, dp0, dp1, dp2, dp3, dq0, dq1, dq2, dq3, ep, eq;
  u64 ap, aq, sp, sq, bq;
  asm("v_add_co_u32 %[sp0], %[ap], %[up0], %[tp0]\n\t"
      "v_sub_co_u32 %[tp0], %[sp], %[up0], %[tp0]\n\t"
      "v_add_co_u32 %[sq0], %[aq], %[uq0], %[tq0]\n\t"
      "v_sub_co_u32 %[tq0], %[sq], %[uq0], %[tq0]\n\t"
      "v_addc_co_u32 %[sp1], %[ap], %[up1], %[tp1], %[ap]\n\t"
      "v_subb_co_u32 %[tp1], %[sp], %[up1], %[tp1], %[sp]\n\t"
      "v_addc_co_u32 %[sq1], %[aq], %[uq1], %[tq1], %[aq]\n\t"
      "v_subb_co_u32 %[tq1], %[sq], %[uq1], %[tq1], %[sq]\n\t"
      "v_addc_co_u32 %[sp2], %[ap], %[up2], %[tp2], %[ap]\n\t"
      "v_subb_co_u32 %[tp2], %[sp], %[up2], %[tp2], %[sp]\n\t"
      "v_addc_co_u32 %[sq2], %[aq], %[uq2], %[tq2], %[aq]\n\t"
      "v_subb_co_u32 %[tq2], %[sq], %[uq2], %[tq2], %[sq]\n\t"
      "v_addc_co_u32 %[sp3], %[ap], %[up3], %[tp3], %[ap]\n\t"  // the carries and borrows out: lane masks
      "v_subb_co_u32 %[tp3], %[sp], %[up3], %[tp3], %[sp]\n\t"
      "v_addc_co_u32 %[sq3], %[aq], %[uq3], %[tq3], %[aq]\n\t"
      "v_subb_co_u32 %[tq3], %[sq], %[uq3], %[tq3], %[sq]\n\t"
      // s - p, p = {1, 0, 0, 0xfffff000}, beside u - t + p under the borrow mask (+ the mask at limb 0, + 0xfffff000 at limb 3)
      "v_subrev_co_u32 %[dp0], vcc, 1, %[sp0]\n\t"
      "v_subrev_co_u32 %[dq0], %[bq], 1, %[sq0]\n\t"
      "v_cndmask_b32 %[ep], 0, %[k], %[sp]\n\t"
      "v_cndmask_b32 %[eq], 0, %[k], %[sq]\n\t"
      "v_subbrev_co_u32 %[dp1], vcc, 0, %[sp1], vcc\n\t"
      "v_subbrev_co_u32 %[dq1], %[bq], 0, %[sq1], %[bq]\n\t"
      "v_addc_co_u32 %[tp0], %[sp], 0, %[tp0], %[sp]\n\t"
      "v_addc_co_u32 %[tq0], %[sq], 0, %[tq0], %[sq]\n\t"
      "v_subbrev_co_u32 %[dp2], vcc, 0, %[sp2], vcc\n\t"
      "v_subbrev_co_u32 %[dq2], %[bq], 0, %[sq2], %[bq]\n\t"
      "v_addc_co_u32 %[tp1], %[sp], 0, %[tp1], %[sp]\n\t"
      "v_addc_co_u32 %[tq1], %[sq], 0, %[tq1], %[sq]\n\t"
      "v_subb_co_u32 %[dp3], vcc, %[sp3], %[k], vcc\n\t"  // final borrow set <=> s < p
      "v_subb_co_u32 %[dq3], %[bq], %[sq3], %[k], %[bq]\n\t"
      "v_addc_co_u32 %[tp2], %[sp], 0, %[tp2], %[sp]\n\t"
      "v_addc_co_u32 %[tq2], %[sq], 0, %[tq2], %[sq]\n\t"
      "s_andn2_b64 vcc, vcc, %[ap]\n\t"  // keep s <=> (c:s) < p <=> borrow and no carry
      "s_andn2_b64 %[bq], %[bq], %[aq]\n\t"
      "v_cndmask_b32 %[dp0], %[dp0], %[sp0], vcc\n\t"
      "v_cndmask_b32 %[dq0], %[dq0], %[sq0], %[bq]\n\t"
      "v_addc_co_u32 %[tp3], %[sp], %[ep], %[tp3], %[sp]\n\t"
      "v_addc_co_u32 %[tq3], %[sq], %[eq], %[tq3], %[sq]\n\t"
      "v_cndmask_b32 %[dp1], %[dp1], %[sp1], vcc\n\t"
      "v_cndmask_b32 %[dq1], %[dq1], %[sq1], %[bq]\n\t"
      "v_cndmask_b32 %[dp2], %[dp2], %[sp2], vcc\n\t"
      "v_cndmask_b32 %[dq2], %[dq2], %[sq2], %[bq]\n\t"
      "v_cndmask_b32 %[dp3], %[dp3], %[sp3], vcc\n\t"
      "v_cndmask_b32 %[dq3], %[dq3], %[sq3], %[bq]"
      : [sp0] "=&v"(sp0), [sp1] "=&v"(sp1), [sp2] "=&v"(sp2), [sp3] "=&v"(sp3), [sq0] "=&v"(sq0), [sq1] "=&v"(sq1), [sq2] "=&v"(sq2),
        [sq3] "=&v"(sq3), [dp0] "=&v"(dp0), [dp1] "=&v"(dp1), [dp2] "=&v"(dp2), [dp3] "=&v"(dp3), [dq0] "=&v"(dq0), [dq1] "=&v"(dq1),
        [dq2] "=&v"(dq2), [dq3] "=&v"(dq3), [tp0] "+v"(tp0), [tp1] "+v"(tp1), [tp2] "+v"(tp2), [tp3] "+v"(tp3), [tq0] "+v"(tq0),
        [tq1] "+v"(tq1), [tq2] "+v"(tq2), [tq3] "+v"(tq3), [ep] "=&v"(ep), [eq] "=&v"(eq), [ap] "=&s"(ap), [aq] "=&s"(aq), [sp] "=&s"(sp),
        [sq] "=&s"(sq), [bq] "=&s"(bq)
      : [up0] "v"(up0), [up1] "v"(up1), [up2] "v"(up2), [up3] "v"(up3), [uq0] "v"(uq0), [uq1] "v"(uq1), [uq2] "v"(uq2), [uq3] "v"(uq3),
        [k] "v"(0xfffff000u)
      : "vcc", "scc");
  xp = FP_PACK(dp0, dp1, dp2, dp3);
  yp = FP_PACK(tp0, tp1, tp2, tp3);
  xq = FP_PACK(dq0, dq1, dq2, dq3);
  yq = FP_PACK(tq0, tq1, tq2, tq3);
}

// One butterfly, (x, y) = (u + t lazy, u - t) for (u, t) = (x, y): the two chains of fpt_bfly2_lazy (VCC and c1), one
// instruction between every link and an `s_nop 0` beside it; the two v_cndmask stand between the masks and their folds.  18 VALU.
// y has registers of its own here: tied to t's, round 0 of pass A copied two limbs of a loaded tuple out of the way.
__device__ __forceinline__ void fpt_bfly_lazy(elt_t& x, elt_t& y) {
  FP_W(x, u0, u1, u2, u3);
  FP_W(y, t0, t1, t2, t3);
  u32 d0, d1, d2, d3, y0, y1, y2, y3, ea, es;
  u64 c1;
  asm("v_add_co_u32 %[d0], vcc, %[u0], %[t0]\n\t"
      "v_sub_co_u32 %[y0], %[c1], %[u0], %[t0]\n\t"
      "s_nop 0\n\t"
      "v_addc_co_u32 %[d1], vcc, %[u1], %[t1], vcc\n\t"
      "v_subb_co_u32 %[y1], %[c1], %[u1], %[t1], %[c1]\n\t"
      "s_nop 0\n\t"
      "v_addc_co_u32 %[d2], vcc, %[u2], %[t2], vcc\n\t"
      "v_subb_co_u32 %[y2], %[c1], %[u2], %[t2], %[c1]\n\t"
      "s_nop 0\n\t"
      "v_addc_co_u32 %[d3], vcc, %[u3], %[t3], vcc\n\t"
      "v_subb_co_u32 %[y3], %[c1], %[u3], %[t3], %[c1]\n\t"
      "s_nop 0\n\t"
      "v_cndmask_b32 %[ea], 0, %[k], vcc\n\t"
      "v_cndmask_b32 %[es], 0, %[k], %[c1]\n\t"
      "v_subbrev_co_u32 %[d0], vcc, 0, %[d0], vcc\n\t"
      "v_addc_co_u32 %[y0], %[c1], 0, %[y0], %[c1]\n\t"
      "s_nop 0\n\t"
      "v_subbrev_co_u32 %[d1], vcc, 0, %[d1], vcc\n\t"
      "v_addc_co_u32 %[y1], %[c1], 0, %[y1], %[c1]\n\t"
      "s_nop 0\n\t"
      "v_subbrev_co_u32 %[d2], vcc, 0, %[d2], vcc\n\t"
      "v_addc_co_u32 %[y2], %[c1], 0, %[y2], %[c1]\n\t"
      "s_nop 0\n\t"
      "v_subb_co_u32 %[d3], vcc, %[d3], %[ea], vcc\n\t"
      "v_addc_co_u32 %[y3], %[c1], %[es], %[y3], %[c1]"
      : [d0] "=&v"(d0), [d1] "=&v"(d1), [d2] "=&v"(d2), [d3] "=&v"(d3), [y0] "=&v"(y0), [y1] "=&v"(y1), [y2] "=&v"(y2), [y3] "=&v"(y3),
        [ea] "=&v"(ea), [es] "=&v"(es), [c1] "=&s"(c1)
      : [u0] "v"(u0), [u1] "v"(u1), [u2] "v"(u2), [u3] "v"(u3), [t0] "v"(t0), [t1] "v"(t1), [t2] "v"(t2), [t3] "v"(t3), [k] "v"(0xfffff000u)
      : "vcc");
  x = FP_PACK(d0, d1, d2, d3);
  y = FP_PACK(y0, y1, y2, y3);
}

// Two values lazy -> canonical, as fpt_canon: p's chain in VCC, q's in c1
__device__ __forceinline__ void fpt_canon2(elt_t& p, elt_t& q) {
  FP_W(p, a0, a1, a2, a3);
  FP_W(q, b0, b1, b2, b3);
  u32 d0, d1, d2, d3, e0, e1, e2, e3;
  u64 c1;
  asm("v_subrev_co_u32 %[d0], vcc, 1, %[a0]\n\t"
      "v_subrev_co_u32 %[e0], %[c1], 1, %[b0]\n\t"
      "s_nop 0\n\t"
      "v_subbrev_co_u32 %[d1], vcc, 0, %[a1], vcc\n\t"
      "v_subbrev_co_u32 %[e1], %[c1], 0, %[b1], %[c1]\n\t"
      "s_nop 0\n\t"
      "v_subbrev_co_u32 %[d2], vcc, 0, %[a2], vcc\n\t"
      "v_subbrev_co_u32 %[e2], %[c1], 0, %[b2], %[c1]\n\t"
      "s_nop 0\n\t"
      "v_subb_co_u32 %[d3], vcc, %[a3], %[k], vcc\n\t"  // borrow <=> the value < p: keep it
      "v_subb_co_u32 %[e3], %[c1], %[b3], %[k], %[c1]\n\t"
      "s_nop 0\n\t"
      "v_cndmask_b32 %[d0], %[d0], %[a0], vcc\n\t"
      "v_cndmask_b32 %[d1], %[d1], %[a1], vcc\n\t"
      "v_cndmask_b32 %[d2], %[d2], %[a2], vcc\n\t"
      "v_cndmask_b32 %[d3], %[d3], %[a3], vcc\n\t"
      "v_cndmask_b32 %[e0], %[e0], %[b0], %[c1]\n\t"
      "v_cndmask_b32 %[e1], %[e1], %[b1], %[c1]\n\t"
      "v_cndmask_b32 %[e2], %[e2], %[b2], %[c1]\n\t"
      "v_cndmask_b32 %[e3], %[e3], %[b3], %[c1]"
      : [d0] "=&v"(d0), [d1] "=&v"(d1), [d2] "=&v"(d2), [d3] "=&v"(d3), [e0] "=&v"(e0), [e1] "=&v"(e1), [e2] "=&v"(e2), [e3] "=&v"(e3),
        [c1] "=&s"(c1)
      : [a0] "v"(a0), [a1] "v"(a1), [a2] "v"(a2), [a3] "v"(a3), [b0] "v"(b0), [b1] "v"(b1), [b2] "v"(b2), [b3] "v"(b3), [k] "v"(0xfffff000u)
      : "vcc");
  p = FP_PACK(d0, d1, d2, d3);
  q = FP_PACK(e0, e1, e2, e3);
}

// The columns of two products P = pa pb and Q = qa qb (FPT_COLUMNS twice), one asm statement per column with both products'
// mads and captures.  Each capturing mad writes its carry to an SGPR pair of its own and the captures follow the column's
// last mad, so every capture stands at least two VALU instructions behind its mad; columns 1 and 5, with one capturing mad per
// product, take an `s_nop 0`.  The bare mads (carry to VCC, never read) and the MADW / MADC distinction are those of FPT_COLUMNS.
// Column 1's addends {acc0.hi, 0} are live together and the compiler keeps one register at zero: p's pair is made in C, as
// FPT_COLUMNS' (one v_mov_b32 into the low half beside that zero), q's by a 64-bit shift in the statement, which needs no zero.
#define FPT_M2 "v_mad_u64_u32 "
#define FPT_C2 "v_addc_co_u32 "
#define FPT_COLUMNS2(C)                                                                                                          \
  asm(FPT_M2 "%[pacc], vcc, %[pa0], %[pb0], 0\n\t"                                                                                \
      FPT_M2 "%[qacc], vcc, %[qa0], %[qb0], 0"                                                                                    \
      : [pacc] "=&v"(pacc0), [qacc] "=&v"(qacc0)                                                                                  \
      : [pa0] "v"(pa0), [pb0] C(pb0), [qa0] "v"(qa0), [qb0] C(qb0)                                                                \
      : "vcc");                                                                                                                   \
  pt0 = (u32)pacc0;                                                                                                               \
  qt0 = (u32)qacc0;                                                                                                               \
  asm("v_lshrrev_b64 %[qin], 32, %[qacc0]\n\t"                                                                                    \
      FPT_M2 "%[pacc], vcc, %[pa0], %[pb1], %[pin]\n\t"                                                                           \
      FPT_M2 "%[qacc], vcc, %[qa0], %[qb1], %[qin]\n\t"                                                                           \
      FPT_M2 "%[pacc], %[s1], %[pa1], %[pb0], %[pacc]\n\t"                                                                        \
      FPT_M2 "%[qacc], %[s2], %[qa1], %[qb0], %[qacc]\n\t"                                                                        \
      "s_nop 0\n\t"                                                                                                               \
      FPT_C2 "%[pov], vcc, 0, 0, %[s1]\n\t"                                                                                       \
      FPT_C2 "%[qov], vcc, 0, 0, %[s2]"                                                                                           \
      : [pacc] "=&v"(pacc), [qacc] "=&v"(qacc), [pov] "=&v"(pov), [qov] "=&v"(qov), [s1] "=&s"(s1), [s2] "=&s"(s2),               \
        [qin] "=&v"(qin)                                                                                                          \
      : [pa0] "v"(pa0), [pa1] "v"(pa1), [pb0] C(pb0), [pb1] C(pb1), [qa0] "v"(qa0), [qa1] "v"(qa1), [qb0] C(qb0), [qb1] C(qb1),   \
        [pin] "v"(pacc0 >> 32), [qacc0] "v"(qacc0)                                                                                \
      : "vcc");                                                                                                                   \
  FPT_COL(pt1, pacc, pov);                                                                                                        \
  FPT_COL(qt1, qacc, qov);                                                                                                        \
  FPT_COLUMN2_3(C, 0, 2, 1, 1, 2, 0);                                                                                             \
  FPT_COL(pt2, pacc, pov);                                                                                                        \
  FPT_COL(qt2, qacc, qov);                                                                                                        \
  asm(FPT_M2 "%[pacc], vcc, %[pa0], %[pb3], %[pacc]\n\t"                                                                          \
      FPT_M2 "%[qacc], vcc, %[qa0], %[qb3], %[qacc]\n\t"                                                                          \
      FPT_M2 "%[pacc], %[s1], %[pa1], %[pb2], %[pacc]\n\t"                                                                        \
      FPT_M2 "%[qacc], %[s2], %[qa1], %[qb2], %[qacc]\n\t"                                                                        \
      FPT_M2 "%[pacc], %[s3], %[pa2], %[pb1], %[pacc]\n\t"                                                                        \
      FPT_M2 "%[qacc], %[s4], %[qa2], %[qb1], %[qacc]\n\t"                                                                        \
      FPT_M2 "%[pacc], %[s5], %[pa3], %[pb0], %[pacc]\n\t"                                                                        \
      FPT_M2 "%[qacc], %[s6], %[qa3], %[qb0], %[qacc]\n\t"                                                                        \
      FPT_C2 "%[pov], vcc, 0, 0, %[s1]\n\t"                                                                                       \
      FPT_C2 "%[qov], vcc, 0, 0, %[s2]\n\t"                                                                                       \
      FPT_C2 "%[pov], vcc, 0, %[pov], %[s3]\n\t"                                                                                  \
      FPT_C2 "%[qov], vcc, 0, %[qov], %[s4]\n\t"                                                                                  \
      FPT_C2 "%[pov], vcc, 0, %[pov], %[s5]\n\t"                                                                                  \
      FPT_C2 "%[qov], vcc, 0, %[qov], %[s6]"                                                                                      \
      : [pacc] "+v"(pacc), [qacc] "+v"(qacc), [pov] "=&v"(pov), [qov] "=&v"(qov), [s1] "=&s"(s1), [s2] "=&s"(s2), [s3] "=&s"(s3), \
        [s4] "=&s"(s4), [s5] "=&s"(s5), [s6] "=&s"(s6)                                                                            \
      : [pa0] "v"(pa0), [pa1] "v"(pa1), [pa2] "v"(pa2), [pa3] "v"(pa3), [pb0] C(pb0), [pb1] C(pb1), [pb2] C(pb2), [pb3] C(pb3),   \
        [qa0] "v"(qa0), [qa1] "v"(qa1), [qa2] "v"(qa2), [qa3] "v"(qa3), [qb0] C(qb0), [qb1] C(qb1), [qb2] C(qb2), [qb3] C(qb3)    \
      : "vcc");                                                                                                                   \
  FPT_COL(pt3, pacc, pov);                                                                                                        \
  FPT_COL(qt3, qacc, qov);                                                                                                        \
  FPT_COLUMN2_3(C, 1, 3, 2, 2, 3, 1);                                                                                             \
  FPT_COL(pt4, pacc, pov);                                                                                                        \
  FPT_COL(qt4, qacc, qov);                                                                                                        \
  asm(FPT_M2 "%[pacc], vcc, %[pa2], %[pb3], %[pacc]\n\t"                                                                          \
      FPT_M2 "%[qacc], vcc, %[qa2], %[qb3], %[qacc]\n\t"                                                                          \
      FPT_M2 "%[pacc], %[s1], %[pa3], %[pb2], %[pacc]\n\t"                                                                        \
      FPT_M2 "%[qacc], %[s2], %[qa3], %[qb2], %[qacc]\n\t"                                                                        \
      "s_nop 0\n\t"                                                                                                               \
      FPT_C2 "%[pov], vcc, 0, 0, %[s1]\n\t"                                                                                       \
      FPT_C2 "%[qov], vcc, 0, 0, %[s2]"                                                                                           \
      : [pacc] "+v"(pacc), [qacc] "+v"(qacc), [pov] "=&v"(pov), [qov] "=&v"(qov), [s1] "=&s"(s1), [s2] "=&s"(s2)                  \
      : [pa2] "v"(pa2), [pa3] "v"(pa3), [pb2] C(pb2), [pb3] C(pb3), [qa2] "v"(qa2), [qa3] "v"(qa3), [qb2] C(qb2), [qb3] C(qb3)    \
      : "vcc");                                                                                                                   \
  FPT_COL(pt5, pacc, pov);                                                                                                        \
  FPT_COL(qt5, qacc, qov);                                                                                                        \
  asm(FPT_M2 "%[pacc], vcc, %[pa3], %[pb3], %[pacc]\n\t"                                                                          \
      FPT_M2 "%[qacc], vcc, %[qa3], %[qb3], %[qacc]"                                                                              \
      : [pacc] "+v"(pacc), [qacc] "+v"(qacc)                                                                                      \
      : [pa3] "v"(pa3), [pb3] C(pb3), [qa3] "v"(qa3), [qb3] C(qb3)                                                                \
      : "vcc");                                                                                                                   \
  pt6 = (u32)pacc;                                                                                                                \
  pt7 = (u32)(pacc >> 32);                                                                                                        \
  qt6 = (u32)qacc;                                                                                                                \
  qt7 = (u32)(qacc >> 32)
// a column of three mads per product, a_i b_j + a_k b_l + a_m b_n (columns 2 and 4): bare, MADW, MADC
#define FPT_COLUMN2_3(C, i, j, k, l, m, n)                                                                                        \
  asm(FPT_M2 "%[pacc], vcc, %[pi], %[pj], %[pacc]\n\t"                                                                            \
      FPT_M2 "%[qacc], vcc, %[qi], %[qj], %[qacc]\n\t"                                                                            \
      FPT_M2 "%[pacc], %[s1], %[pk], %[pl], %[pacc]\n\t"                                                                          \
      FPT_M2 "%[qacc], %[s2], %[qk], %[ql], %[qacc]\n\t"                                                                          \
      FPT_M2 "%[pacc], %[s3], %[pm], %[pn], %[pacc]\n\t"                                                                          \
      FPT_M2 "%[qacc], %[s4], %[qm], %[qn], %[qacc]\n\t"                                                                          \
      FPT_C2 "%[pov], vcc, 0, 0, %[s1]\n\t"                                                                                       \
      FPT_C2 "%[qov], vcc, 0, 0, %[s2]\n\t"                                                                                       \
      FPT_C2 "%[pov], vcc, 0, %[pov], %[s3]\n\t"                                                                                  \
      FPT_C2 "%[qov], vcc, 0, %[qov], %[s4]"                                                                                      \
      : [pacc] "+v"(pacc), [qacc] "+v"(qacc), [pov] "=&v"(pov), [qov] "=&v"(qov), [s1] "=&s"(s1), [s2] "=&s"(s2), [s3] "=&s"(s3), \
        [s4] "=&s"(s4)                                                                                                            \
      : [pi] "v"(pa##i), [pk] "v"(pa##k), [pm] "v"(pa##m), [pj] C(pb##j), [pl] C(pb##l), [pn] C(pb##n), [qi] "v"(qa##i),          \
        [qk] "v"(qa##k), [qm] "v"(qa##m), [qj] C(qb##j), [ql] C(qb##l), [qn] C(qb##n)                                             \
      : "vcc")

// Two products, a w / 2^128 mod p each as fpt_mul_t (same schedule per product, same preconditions: pw, qw < p, and
// wave-uniform under SW), instruction for instruction.  The reduction is one statement: p's chains run in VCC, q's in the pair
// qs; the shifts U >> 20 stand between the links of the two T_hi - U chains (each overwrites a limb of U behind its last reader)
// and the two v_cndmask between the first links of the + p chains; the links of + (U >> 20) + cy have one instruction between them
// and an `s_nop 0`.  One s_andn2_b64 per product, as before, two instructions behind the mask's VALU write.
template <bool SW>
__device__ __forceinline__ void fpt_mul2_t(elt_t& pa, elt_t pw, elt_t& qa, elt_t qw) {
  FP_W(pa, pa0, pa1, pa2, pa3);
  FP_W(pw, pb0, pb1, pb2, pb3);
  FP_W(qa, qa0, qa1, qa2, qa3);
  FP_W(qw, qb0, qb1, qb2, qb3);
  u32 pt0, pt1, pt2, pt3, pt4, pt5, pt6, pt7, pov, qt0, qt1, qt2, qt3, qt4, qt5, qt6, qt7, qov;
  u64 pacc0, pacc, qacc0, qacc, qin, s1, s2, s3, s4, s5, s6;
  if constexpr (SW) {
    FPT_COLUMNS2("s");
  } else {
    FPT_COLUMNS2("v");
  }
  const u32 pk = pt0 << 12, qk = qt0 << 12;
  u32 pd0, pd1, pd2, pd3, qd0, qd1, qd2, qd3, pe, qe;
  u64 pcy, pb, qcy, qb, qs;
  asm("v_add_co_u32 %[pt3], %[pcy], %[pt3], %[pk]\n\t"  // u3 (in t3's register), cy
      "v_add_co_u32 %[qt3], %[qcy], %[qt3], %[qk]\n\t"
      "v_sub_co_u32 %[pd0], vcc, %[pt4], %[pt0]\n\t"  // T_hi - U
      "v_sub_co_u32 %[qd0], %[qs], %[qt4], %[qt0]\n\t"
      "v_alignbit_b32 %[pt0], %[pt1], %[pt0], 20\n\t"  // U >> 20, in U's registers
      "v_alignbit_b32 %[qt0], %[qt1], %[qt0], 20\n\t"
      "v_subb_co_u32 %[pd1], vcc, %[pt5], %[pt1], vcc\n\t"
      "v_subb_co_u32 %[qd1], %[qs], %[qt5], %[qt1], %[qs]\n\t"
      "v_alignbit_b32 %[pt1], %[pt2], %[pt1], 20\n\t"
      "v_alignbit_b32 %[qt1], %[qt2], %[qt1], 20\n\t"
      "v_subb_co_u32 %[pd2], vcc, %[pt6], %[pt2], vcc\n\t"
      "v_subb_co_u32 %[qd2], %[qs], %[qt6], %[qt2], %[qs]\n\t"
      "v_alignbit_b32 %[pt2], %[pt3], %[pt2], 20\n\t"
      "v_alignbit_b32 %[qt2], %[qt3], %[qt2], 20\n\t"
      "v_subb_co_u32 %[pd3], %[pb], %[pt7], %[pt3], vcc\n\t"  // borrow-out: lane masks pb, qb
      "v_subb_co_u32 %[qd3], %[qb], %[qt7], %[qt3], %[qs]\n\t"
      "v_lshrrev_b32 %[pt3], 20, %[pt3]\n\t"
      "v_lshrrev_b32 %[qt3], 20, %[qt3]\n\t"
      "v_addc_co_u32 %[pd0], vcc, %[pd0], %[pt0], %[pcy]\n\t"  // + (U >> 20) + cy, cy the carry-in
      "v_addc_co_u32 %[qd0], %[qs], %[qd0], %[qt0], %[qcy]\n\t"
      "s_nop 0\n\t"
      "v_addc_co_u32 %[pd1], vcc, %[pd1], %[pt1], vcc\n\t"
      "v_addc_co_u32 %[qd1], %[qs], %[qd1], %[qt1], %[qs]\n\t"
      "s_nop 0\n\t"
      "v_addc_co_u32 %[pd2], vcc, %[pd2], %[pt2], vcc\n\t"
      "v_addc_co_u32 %[qd2], %[qs], %[qd2], %[qt2], %[qs]\n\t"
      "s_nop 0\n\t"
      "v_addc_co_u32 %[pd3], %[pcy], %[pd3], %[pt3], vcc\n\t"  // carry-out: lane masks c (in cy's SGPR pairs)
      "v_addc_co_u32 %[qd3], %[qcy], %[qd3], %[qt3], %[qs]\n\t"
      "s_nop 0\n\t"
      "s_andn2_b64 %[pcy], %[pb], %[pcy]\n\t"  // W < 0 <=> b and no c
      "s_andn2_b64 %[qcy], %[qb], %[qcy]\n\t"
      // W < 0 => + p: + 1 at limb 0 (the mask is the carry-in), + 0xfffff000 at limb 3
      "v_addc_co_u32 %[pd0], vcc, 0, %[pd0], %[pcy]\n\t"
      "v_addc_co_u32 %[qd0], %[qs], 0, %[qd0], %[qcy]\n\t"
      "v_cndmask_b32 %[pe], 0, %[k], %[pcy]\n\t"
      "v_cndmask_b32 %[qe], 0, %[k], %[qcy]\n\t"
      "v_addc_co_u32 %[pd1], vcc, 0, %[pd1], vcc\n\t"
      "v_addc_co_u32 %[qd1], %[qs], 0, %[qd1], %[qs]\n\t"
      "s_nop 0\n\t"
      "v_addc_co_u32 %[pd2], vcc, 0, %[pd2], vcc\n\t"
      "v_addc_co_u32 %[qd2], %[qs], 0, %[qd2], %[qs]\n\t"
      "s_nop 0\n\t"
      "v_addc_co_u32 %[pd3], vcc, %[pe], %[pd3], vcc\n\t"
      "v_addc_co_u32 %[qd3], %[qs], %[qe], %[qd3], %[qs]"
      : [pd0] "=&v"(pd0), [pd1] "=&v"(pd1), [pd2] "=&v"(pd2), [pd3] "=&v"(pd3), [qd0] "=&v"(qd0), [qd1] "=&v"(qd1), [qd2] "=&v"(qd2),
        [qd3] "=&v"(qd3), [pt0] "+v"(pt0), [pt1] "+v"(pt1), [pt2] "+v"(pt2), [pt3] "+v"(pt3), [qt0] "+v"(qt0), [qt1] "+v"(qt1),
        [qt2] "+v"(qt2), [qt3] "+v"(qt3), [pe] "=&v"(pe), [qe] "=&v"(qe), [pcy] "=&s"(pcy), [pb] "=&s"(pb), [qcy] "=&s"(qcy),
        [qb] "=&s"(qb), [qs] "=&s"(qs)
      : [pk] "v"(pk), [qk] "v"(qk), [k] "v"(0xfffff000u), [pt4] "v"(pt4), [pt5] "v"(pt5), [pt6] "v"(pt6), [pt7] "v"(pt7), [qt4] "v"(qt4),
        [qt5] "v"(qt5), [qt6] "v"(qt6), [qt7] "v"(qt7)
      : "vcc", "scc");
  // pt0..pt3 and qt0..qt3 hold U >> 20 from here on
  pa = FP_PACK(pd0, pd1, pd2, pd3);
  qa = FP_PACK(qd0, qd1, qd2, qd3);
}
__device__ __forceinline__ void fpt_mul2(elt_t& pa, elt_t pw, elt_t& qa, elt_t qw) { fpt_mul2_t<false>(pa, pw, qa, qw); }
__device__ __forceinline__ void fpt_mul2_sw(elt_t& pa, elt_t pw, elt_t& qa, elt_t qw) { fpt_mul2_t<true>(pa, pw, qa, qw); }
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
// the paired routines: the single ones twice
LF_HD void fpt_bfly_lazy(elt_t& x, elt_t& y) {
  const elt_t u = x, t = y;
  x = fpt_add_lazy(u, t);
  y = fpt_sub(u, t);
}
LF_HD void fpt_bfly2_lazy(elt_t& xp, elt_t& yp, elt_t& xq, elt_t& yq) {
  fpt_bfly_lazy(xp, yp);
  fpt_bfly_lazy(xq, yq);
}
LF_HD void fpt_canon2(elt_t& p, elt_t& q) {
  p = fpt_canon(p);
  q = fpt_canon(q);
}
LF_HD void fpt_bfly2_full(elt_t& xp, elt_t& yp, elt_t& xq, elt_t& yq) {
  const elt_t up = xp, tp = yp, uq = xq, tq = yq;
  xp = fpt_add(up, tp), yp = fpt_sub(up, tp);
  xq = fpt_add(uq, tq), yq = fpt_sub(uq, tq);
}
LF_HD void fpt_mul2(elt_t& pa, elt_t pw, elt_t& qa, elt_t qw) {
  pa = fpt_mul(pa, pw);
  qa = fpt_mul(qa, qw);
}
LF_HD void fpt_mul2_sw(elt_t& pa, elt_t pw, elt_t& qa, elt_t qw) { fpt_mul2(pa, pw, qa, qw); }
#endif
