// zk256.hip -- ZkProver<Fp256Base, .> on the device: the P-256 base-field half of BASELINE config 5 (the mdoc signature
// circuit: 21 layers, 4.8e5 terms, 32-byte elements, lib/circuits/mdoc/mdoc_zk.cc:70-76,485-522).
//
// Same algorithms as the 16-byte fields, restated over elt32_t (fp256.h) with the straightforward kernel structure -- the
// circuit is small (layers of 2^9 .. 2^16 wires), so every round-hand is a handful of short launches and ONE read-back:
//   eval_circuit            ProverLayers::eval_quad            lib/sumcheck/prover_layers.h:278-305
//   bind_g                  Quad::bind_g + Eqs::raw_eq2        lib/sumcheck/quad.h:152-185, lib/arrays/eqs.h:46-80
//   round body              ProverLayers::layer / evaluations  lib/sumcheck/prover_layers.h:230-263,357-402
//   binds                   Dense::bind, HQuad::bind_h         lib/arrays/dense.h:70-87, lib/sumcheck/hquad.h:90-123
//   Ligero                  LigeroProver::commit / prove       lib/ligero/ligero_prover.h:58-146,171-351
//   driver                  ZkProver::commit (lib/zk/zk_prover.h:72-96) here; prove, verifier_constraints, ZkProof::write / read
//                           and the verifier are csrc/zk_proto.h, instantiated with the policy P32 at the end of this file
//   batch                   B provers in lock-step: zkp::prove_batch<P32> (zk_proto.h) over the *_batch kernels here, Zk256Batch,
//                           lig::prove_batch / open_batch over L32 (lfgpu_zk_prove_batch256, lfgpu_ligero_prove_batch256 / _open_batch256)
// Sums over many terms (run sums of bind_g, the QW scatter) add the 32-bit limbs of canonical residues into 64-bit integer
// accumulators with atomics and reduce once (fp256_reduce_limbs): exact and independent of arrival order, as for Fp128.
// Row extension and column hashing are csrc/p256.hip.
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <string>

#include "ligero_slab.h"  // the Ligero prover record, its commit and prove side (and the host layout), over the policy L32 below
#include "zk_driver.h"  // zk_proto.h -- F256 (the host field), the protocol layer and Wire32 -- and the driver layer around it

typedef elt32_t E;
#define Z_THREADS 256

namespace {
// ------------------------------------------------------------------ kernels
__device__ __forceinline__ void limbs_atomic_add(u64* a, const E& v) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    atomicAdd(&a[2 * k], (u64)(u32)v.l[k]);
    atomicAdd(&a[2 * k + 1], v.l[k] >> 32);
  }
}
// One term per lane; runs of equal keys among consecutive lanes (canonical order keeps equal hand pairs, and mostly also the
// hot target -- the constant wire 0 -- adjacent) are summed inside the wave first, so that a run costs 8 atomics per wave
// instead of 8 per term: the signature circuit has runs of 3e4 terms and one wire that 1e5 terms of a layer read.
// key 0xffffffff marks an idle lane.  Every lane of the wave must call this.
__device__ __forceinline__ void run_fold_commit256(u32 key, E t, u64* __restrict__ acc) {
  const u32 lane = threadIdx.x & 63;
  const u32 pkey = __shfl_up(key, 1, 64);
  const bool head = lane == 0 || pkey != key || key == 0xffffffffu;  // idle lanes never form a run: a partly filled wave skips the fold
  const u64 hmask = __ballot(head);
  if (hmask != ~0ull) {  // wave-uniform: some neighbours share a key
    const u32 rid = (u32)__popcll(hmask & ((2ull << lane) - 1));  // monotone, so equal ids = one contiguous run
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      E o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o.l[k] = __shfl_down(t.l[k], off, 64);
      const u32 orid = __shfl_down(rid, off, 64);
      if (lane + off < 64 && orid == rid) t = fp256_add(t, o);
    }
  }
  if (head && key != 0xffffffffu) limbs_atomic_add(acc + 8 * (size_t)key, t);
}
__device__ __forceinline__ E take_acc256(u64* __restrict__ acc, size_t i, const E& rsq) {
  u64 a[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a[k] = acc[8 * i + k];
    acc[8 * i + k] = 0;
  }
  return fp256_reduce_limbs(a, rsq);
}
// out[i] = the field element of accumulator i; the accumulators are left zeroed (they serve the next sum)
__global__ __launch_bounds__(Z_THREADS) void limb_normalize256_kernel(size_t n, u64* __restrict__ acc, E rsq, E* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * Z_THREADS + threadIdx.x;
  if (i >= n) return;
  st32(&out[i], take_acc256(acc, i, rsq));
}
// ... of statement blockIdx.y: its accumulators at acc + y * s_acc words, its elements at out + y * s_out
__global__ __launch_bounds__(Z_THREADS) void limb_normalize256_batch_kernel(size_t n, u64* __restrict__ acc, size_t s_acc, E rsq, E* __restrict__ out, size_t s_out) {
  const size_t i = (size_t)blockIdx.x * Z_THREADS + threadIdx.x;
  if (i >= n) return;
  st32(&out[(size_t)blockIdx.y * s_out + i], take_acc256(acc + (size_t)blockIdx.y * s_acc, i, rsq));
}

// K11: V[g] = sum_{terms of g} kvec[vi] * W[h1] * W[h0]; assert-zero terms must vanish.  One term per lane over the
// by-gate order (a gate's terms are contiguous: one gate of the signature circuit has 769), summed as above.
__device__ __forceinline__ void eval_quad256_body(size_t n, const corner4* __restrict__ terms, const E* __restrict__ kvec, const E* __restrict__ W,
                                                  u64* __restrict__ acc, int* __restrict__ fail) {
  const size_t i = (size_t)blockIdx.x * Z_THREADS + threadIdx.x;
  u32 key = 0xffffffffu;
  E t = e32_zero();
  if (i < n) {
    const corner4 cr = terms[i];
    key = cr.g;
    const E v = ld32(&kvec[cr.vi]);
    const E p = fp256_mul(ld32(&W[cr.h1]), ld32(&W[cr.h0]));
    if (e32_is_zero(v)) {
      if (!e32_is_zero(p)) atomicOr(fail, 1);
    } else {
      t = fp256_mul(v, p);
    }
  }
  run_fold_commit256(key, t, acc);
}
__global__ __launch_bounds__(Z_THREADS) void eval_quad256_kernel(size_t n, const corner4* __restrict__ terms, const E* __restrict__ kvec,
                                                                 const E* __restrict__ W, u64* __restrict__ acc, int* __restrict__ fail) {
  eval_quad256_body(n, terms, kvec, W, acc, fail);
}
// statement blockIdx.y of a batch: its wires at W + y * ldw, its accumulators at acc + y * s_acc words, its flag fail[y]
__global__ __launch_bounds__(Z_THREADS) void eval_quad256_batch_kernel(size_t n, const corner4* __restrict__ terms, const E* __restrict__ kvec,
                                                                       const E* __restrict__ W, size_t ldw, u64* __restrict__ acc, size_t s_acc,
                                                                       int* __restrict__ fail) {
  eval_quad256_body(n, terms, kvec, W + (size_t)blockIdx.y * ldw, acc + (size_t)blockIdx.y * s_acc, fail + blockIdx.y);
}

// ---- inner_product_vector from a caller's term list (LigeroCommon::inner_product_vector, ligero_param.h:382-421), the step of
// lfgpu_ligero_prove256 / lfgpu_ligero_verify256: terms in any order, duplicates allowed, one wire read by thousands of terms the
// normal case.  The contract of a_terms_fp_kernel (ligero.hip) over 32-byte elements: the product k * alphal[c] of every term goes
// into the accumulators of flat position w of A -- eight 64-bit sums of 32-bit limbs, the 64 contiguous bytes acc[8 w .. 8 w + 8)
// -- with integer atomic adds, after the runs of equal w in lane order have been folded in the wave (run_fold_commit256: one run
// head per entry issues the eight adds); then one fp256_reduce_limbs per entry.  Exact and independent of term and arrival order.
// Summands per entry: every atomic adds the limbs of ONE canonical residue (a product, a folded run, or +-alphaq), so an entry
// that has taken N adds holds limb sums <= N (2^32 - 1) and a total S < N 2^256.  fp256_reduce_limbs wants every limb sum to fit
// 64 bits (N <= 2^32) and the part of S above 2^256 below 2^40 (N <= 2^40): N < 2^32 serves both.  The worst entry takes every
// term and both copy terms of every quadratic triple, so the host refuses nllterm + 6 nq >= 2^32 (lfgpu_zk.h).
struct llterm256_t {  // the memory image of lfgpu_ligero_llterm256
  u64 c, w;
  E k;
};
static_assert(sizeof(llterm256_t) == 48 && sizeof(lfgpu_ligero_llterm256) == 48 && sizeof(size_t) == 8, "lfgpu_ligero_llterm256 is uploaded as it stands");
#define AT256_THREADS 256
#define AT256_BLOCKS_MAX 1024  // grid stride: AT256_THREADS * AT256_BLOCKS_MAX terms per sweep
__global__ __launch_bounds__(AT256_THREADS) void a_terms256_kernel(size_t n, const llterm256_t* __restrict__ t, const E* __restrict__ alphal,
                                                                   u64* __restrict__ acc) {
  const size_t stride = (size_t)gridDim.x * AT256_THREADS;
  for (size_t base = (size_t)blockIdx.x * AT256_THREADS; base < n; base += stride) {  // wave-uniform trip count: the fold shuffles
    const size_t i = base + threadIdx.x;
    u32 key = 0xffffffffu;
    E v = e32_zero();
    if (i < n) {
      const uint4 cw = *reinterpret_cast<const uint4*>(&t[i]);  // c | w (the record is 48 bytes: 16-byte aligned)
      key = cw.z;                                                // w < nw < 2^28 (LigeroParam), checked on the host
      v = fp256_mul(ld32(&t[i].k), ld32(&alphal[(u64)cw.x | ((u64)cw.y << 32)]));
    }
    run_fold_commit256(key, v, acc);
  }
}
// the quadratic copy constraints: A[a0 + j * step + iw] += aq, A[lqc[iw][j]] -= aq for aq = alphaq[iw][j], j < 3
__global__ __launch_bounds__(Z_THREADS) void a_terms_quad256_kernel(u32 n3 /* 3 nq */, const u64* __restrict__ lqc, const E* __restrict__ alphaq, u64 a0, u64 step,
                                                                    u64* __restrict__ acc) {
  const u32 t = blockIdx.x * Z_THREADS + threadIdx.x;
  if (t >= n3) return;
  const u32 iw = t / 3, j = t % 3;
  const E aq = ld32(&alphaq[t]);
  limbs_atomic_add(acc + 8 * (size_t)(a0 + (u64)j * step + iw), aq);
  limbs_atomic_add(acc + 8 * (size_t)lqc[t], fp256_sub(e32_zero(), aq));
}
// rows[i][r + j] += the sum standing in the accumulators of flat position i * w + j
__global__ __launch_bounds__(Z_THREADS) void a_terms_finish256_kernel(u32 r, u32 w, size_t ld, size_t nflat, const u64* __restrict__ acc, E rsq,
                                                                      E* __restrict__ rows) {
  const size_t f = (size_t)blockIdx.x * Z_THREADS + threadIdx.x;
  if (f >= nflat) return;
  u64 a[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = acc[8 * f + k];
  E* dst = &rows[(f / w) * ld + r + f % w];
  st32(dst, fp256_add(ld32(dst), fp256_reduce_limbs(a, rsq)));
}

// eq[i] = EQ(G0, i) + alpha EQ(G1, i), EQ(G, i) = prod_l (bit_l(i) ? G[l] : 1 - G[l]); G = G0 | G1 | 1-G0 | 1-G1
__device__ __forceinline__ void raw_eq2_256_body(u32 logn, u32 n, const E* __restrict__ G, const E& alpha, const E& one, E* __restrict__ eq) {
  const u32 i = blockIdx.x * Z_THREADS + threadIdx.x;
  if (i >= n) return;
  E e0 = one, e1 = alpha;
  for (u32 l = 0; l < logn; ++l) {
    const u32 bit = (i >> l) & 1;
    e0 = fp256_mul(e0, ld32(&G[(bit ? 0 : 2 * logn) + l]));
    e1 = fp256_mul(e1, ld32(&G[(bit ? logn : 3 * logn) + l]));
  }
  st32(&eq[i], fp256_add(e0, e1));
}
__global__ __launch_bounds__(Z_THREADS) void raw_eq2_256_kernel(u32 logn, u32 n, const E* __restrict__ G, E alpha, E one, E* __restrict__ eq) {
  raw_eq2_256_body(logn, n, G, alpha, one, eq);
}
// The batch twins of the EQ kernels: statement blockIdx.y has its point table at G + y * gs (the table of raw_eq2_256 followed by
// the statement's alpha at 4 logn and its beta at 4 logn + 1), its factor tables at tab + y * ts, its vector at eq + y * n
__global__ __launch_bounds__(Z_THREADS) void raw_eq2_256_batch_kernel(u32 logn, u32 n, const E* __restrict__ G, size_t gs, E one, E* __restrict__ eq) {
  const E* Gb = G + (size_t)blockIdx.y * gs;
  raw_eq2_256_body(logn, n, Gb, ld32(&Gb[4 * logn]), one, eq + (size_t)blockIdx.y * n);
}

// The same vector with 2 products per entry instead of 2 logn: EQ(G, i) = LO[i mod 2^lb] * HI[i >> lb].  eq_tables256_kernel
// builds the four factor tables LO0 | HI0 | LO1 | HI1 (alpha folded into HI1), one thread per entry (<= 2^ceil(logn / 2)
// entries each), raw_eq2_split256_kernel combines them.  Exact field arithmetic: the association does not matter.
__device__ __forceinline__ void eq_tables256_body(u32 logn, u32 lb, const E* __restrict__ G, const E& alpha, const E& one, E* __restrict__ tab) {
  const u32 hb = logn - lb, nlo = 1u << lb, nhi = 1u << hb;
  const u32 t = blockIdx.x * Z_THREADS + threadIdx.x;
  if (t >= 2 * (nlo + nhi)) return;
  const u32 which = t < nlo ? 0 : t < nlo + nhi ? 1 : t < 2 * nlo + nhi ? 2 : 3;  // LO0, HI0, LO1, HI1
  const u32 j = which == 0 ? t : which == 1 ? t - nlo : which == 2 ? t - nlo - nhi : t - 2 * nlo - nhi;
  const u32 bits = (which & 1) ? hb : lb, shift = (which & 1) ? lb : 0, g = which >> 1;  // g: 0 -> G0, 1 -> G1
  E e = which == 3 ? alpha : one;
  for (u32 l = 0; l < bits; ++l) {
    const u32 bit = (j >> l) & 1;
    e = fp256_mul(e, ld32(&G[(bit ? g * logn : (2 + g) * logn) + shift + l]));
  }
  st32(&tab[t], e);
}
__global__ __launch_bounds__(Z_THREADS) void eq_tables256_kernel(u32 logn, u32 lb, const E* __restrict__ G, E alpha, E one, E* __restrict__ tab) {
  eq_tables256_body(logn, lb, G, alpha, one, tab);
}
__global__ __launch_bounds__(Z_THREADS) void eq_tables256_batch_kernel(u32 logn, u32 lb, const E* __restrict__ G, size_t gs, E one, E* __restrict__ tab, size_t ts) {
  const E* Gb = G + (size_t)blockIdx.y * gs;
  eq_tables256_body(logn, lb, Gb, ld32(&Gb[4 * logn]), one, tab + (size_t)blockIdx.y * ts);
}
__device__ __forceinline__ void raw_eq2_split256_body(u32 logn, u32 lb, u32 n, const E* __restrict__ tab, E* __restrict__ eq) {
  const u32 i = blockIdx.x * Z_THREADS + threadIdx.x;
  if (i >= n) return;
  const u32 nlo = 1u << lb, nhi = 1u << (logn - lb);
  const u32 lo = i & (nlo - 1), hi = i >> lb;
  const E e0 = fp256_mul(ld32(&tab[lo]), ld32(&tab[nlo + hi]));
  const E e1 = fp256_mul(ld32(&tab[nlo + nhi + lo]), ld32(&tab[2 * nlo + nhi + hi]));
  st32(&eq[i], fp256_add(e0, e1));
}
__global__ __launch_bounds__(Z_THREADS) void raw_eq2_split256_kernel(u32 logn, u32 lb, u32 n, const E* __restrict__ tab, E* __restrict__ eq) {
  raw_eq2_split256_body(logn, lb, n, tab, eq);
}
__global__ __launch_bounds__(Z_THREADS) void raw_eq2_split256_batch_kernel(u32 logn, u32 lb, u32 n, const E* __restrict__ tab, size_t ts, E* __restrict__ eq) {
  raw_eq2_split256_body(logn, lb, n, tab + (size_t)blockIdx.y * ts, eq + (size_t)blockIdx.y * n);
}

// Quad::bind_g: every term computes prep_v(v, beta) * eq[g]; the terms of a run (equal hand pair, contiguous in canonical
// order) add into the run's limb accumulators
__device__ __forceinline__ bool is_head256(const corner4* t, size_t i) { return i == 0 || t[i].h0 != t[i - 1].h0 || t[i].h1 != t[i - 1].h1; }
// WRITE_HC = false (statements b > 0 of a batch): the corners are circuit constants, the same for every statement -- only
// statement 0 writes them (as K14's kernels do, sumcheck.hip)
template <bool WRITE_HC>
__device__ __forceinline__ void bindg_emit256_body(u32* wave_off, size_t n, const corner4* __restrict__ t, const E* __restrict__ kvec, const E* __restrict__ eq,
                                                   const E& beta, const u32* __restrict__ block_off, uint2* __restrict__ hc_out, u64* __restrict__ acc) {
  const size_t i = (size_t)blockIdx.x * BG_THREADS + threadIdx.x;
  const bool valid = i < n;
  const bool head = valid && is_head256(t, i);
  const u64 mask = __ballot(head);
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_off[wave] = (u32)__popcll(mask);
  __syncthreads();
  u32 ri = block_off[blockIdx.x];
  for (u32 w = 0; w < wave; ++w) ri += wave_off[w];
  ri += (u32)__popcll(mask & ((2ull << lane) - 1)) - 1;
  E pv = e32_zero();
  if (valid) {
    const corner4 c0 = t[i];
    E v = ld32(&kvec[c0.vi]);
    if (e32_is_zero(v)) v = beta;
    pv = fp256_mul(v, ld32(&eq[c0.g]));
    if (WRITE_HC && head) hc_out[ri] = make_uint2(c0.h0, c0.h1);
  }
  run_fold_commit256(valid ? ri : 0xffffffffu, pv, acc);
}
__global__ __launch_bounds__(BG_THREADS) void bindg_emit256_kernel(size_t n, const corner4* __restrict__ t, const E* __restrict__ kvec,
                                                                   const E* __restrict__ eq, E beta, const u32* __restrict__ block_off,
                                                                   uint2* __restrict__ hc_out, u64* __restrict__ acc) {
  __shared__ u32 wave_off[BG_THREADS / 64];
  bindg_emit256_body<true>(wave_off, n, t, kvec, eq, beta, block_off, hc_out, acc);
}
// statement blockIdx.y: its EQ vector at eq + y * nv, its beta in its point table (G + y * gs)[ibeta], its run accumulators at
// acc + y * s_acc words -- no two statements share an accumulator
__global__ __launch_bounds__(BG_THREADS) void bindg_emit256_batch_kernel(size_t n, const corner4* __restrict__ t, const E* __restrict__ kvec,
                                                                         const E* __restrict__ eq, size_t nv, const E* __restrict__ G, size_t gs, u32 ibeta,
                                                                         const u32* __restrict__ block_off, uint2* __restrict__ hc_out, u64* __restrict__ acc,
                                                                         size_t s_acc) {
  __shared__ u32 wave_off[BG_THREADS / 64];
  const size_t b = blockIdx.y;
  const E beta = ld32(&G[b * gs + ibeta]);
  if (b == 0) bindg_emit256_body<true>(wave_off, n, t, kvec, eq, beta, block_off, hc_out, acc);
  else bindg_emit256_body<false>(wave_off, n, t, kvec, eq + b * nv, beta, block_off, hc_out, acc + b * s_acc);
}

// QW[h[hand]] += v * Wother[h[1-hand]]
__device__ __forceinline__ void qw_scatter256_body(size_t blk, size_t n, const uint2* __restrict__ hc, const E* __restrict__ vc, int hand,
                                                   const E* __restrict__ Wo, u64* __restrict__ acc) {
  const size_t i = blk * Z_THREADS + threadIdx.x;
  u32 key = 0xffffffffu;
  E t = e32_zero();
  if (i < n) {
    const uint2 h = hc[i];
    key = hand ? h.y : h.x;
    t = fp256_mul(ld32(&vc[i]), ld32(&Wo[hand ? h.x : h.y]));
  }
  run_fold_commit256(key, t, acc);
}
__global__ __launch_bounds__(Z_THREADS) void qw_scatter256_kernel(size_t n, const uint2* __restrict__ hc, const E* __restrict__ vc, int hand,
                                                                  const E* __restrict__ Wo, u64* __restrict__ acc) {
  qw_scatter256_body(blockIdx.x, n, hc, vc, hand, Wo, acc);
}
// statement blockIdx.y: shared corners, its values at vc + y * s_vc, the other hand at Wo + y * s_wo, its targets at acc + y * s_acc words
__global__ __launch_bounds__(Z_THREADS) void qw_scatter256_batch_kernel(size_t n, const uint2* __restrict__ hc, const E* __restrict__ vc, size_t s_vc, int hand,
                                                                        const E* __restrict__ Wo, size_t s_wo, u64* __restrict__ acc, size_t s_acc) {
  const size_t b = blockIdx.y;
  qw_scatter256_body(blockIdx.x, n, hc, vc + b * s_vc, hand, Wo + b * s_wo, acc + b * s_acc);
}

__device__ __forceinline__ E block_sum256(E v, E* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (u32 s = Z_THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = fp256_add(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  const E r = sh[0];
  __syncthreads();
  return r;
}
// The two sums of a round (ProverLayers::evaluations :357-402), a0 = sum QW[2i] W[2i] and
// a2 = sum (QW[2i+1] - QW[2i]) (W[2i+1] - W[2i]), straight from the scatter's limb accumulators: every accumulator is
// reduced to its field element here and zeroed for the next round-hand; the block sums go, again as limbs, into 16 words
// (out[0..8) = a0, out[8..16) = a2) that the host reduces.
// post != nullptr: the block that finishes last copies the 16 words to coherent pinned host memory (post[0..16)), clears
// them and publishes `seq` at post[16] -- the host spins on that word instead of a copy + stream synchronisation.
// the two sums of this thread over the pairs of blocks blk, blk + nblk, ...  (acc: the scatter's accumulators, left zeroed)
__device__ __forceinline__ void partials256_thread(size_t blk, size_t nblk, size_t n, u64* __restrict__ acc, const E& rsq, const E* __restrict__ W, E& a0, E& a2) {
  const size_t nodd = n / 2;
  for (size_t i = blk * Z_THREADS + threadIdx.x; i < nodd; i += nblk * Z_THREADS) {
    const E q0 = take_acc256(acc, 2 * i, rsq), q1 = take_acc256(acc, 2 * i + 1, rsq), w0 = ld32(&W[2 * i]), w1 = ld32(&W[2 * i + 1]);
    a0 = fp256_add(a0, fp256_mul(q0, w0));
    a2 = fp256_add(a2, fp256_mul(fp256_sub(q1, q0), fp256_sub(w1, w0)));
  }
  if (blk == 0 && threadIdx.x == 0 && 2 * nodd < n) {  // odd tail (:381-388)
    const E t = fp256_mul(take_acc256(acc, 2 * nodd, rsq), ld32(&W[2 * nodd]));
    a0 = fp256_add(a0, t);
    a2 = fp256_add(a2, t);
  }
}
__device__ __forceinline__ void partials256_body(E* sh, u32* s_last, size_t n, u64* __restrict__ acc, const E& rsq, const E* __restrict__ W, u64* __restrict__ out,
                                                 u32* __restrict__ done, volatile u64* __restrict__ post, u64 seq) {
  E a0 = e32_zero(), a2 = e32_zero();
  partials256_thread(blockIdx.x, gridDim.x, n, acc, rsq, W, a0, a2);
  a0 = block_sum256(a0, sh);
  a2 = block_sum256(a2, sh);
  if (threadIdx.x == 0) {
    limbs_atomic_add(out, a0);
    limbs_atomic_add(out + 8, a2);
    *s_last = 0;
    if (post) {
      __threadfence();
      *s_last = atomicAdd(done, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
  }
  __syncthreads();
  if (*s_last && threadIdx.x < 64) {  // every block's adds are visible (each fenced before its increment); 16 lanes of one wave read,
    if (threadIdx.x < 16) {          // clear and copy one word each (the round trips overlap), lane 0 then publishes
      post[threadIdx.x] = __hip_atomic_exchange(&out[threadIdx.x], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
    }
    if (threadIdx.x == 0) {
      *done = 0;
      __hip_atomic_store((u64*)&post[16], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
__global__ __launch_bounds__(Z_THREADS) void partials256_kernel(size_t n, u64* __restrict__ acc, E rsq, const E* __restrict__ W, u64* __restrict__ out,
                                                                u32* __restrict__ done, volatile u64* __restrict__ post, u64 seq) {
  __shared__ E sh[Z_THREADS];
  __shared__ u32 s_last;
  partials256_body(sh, &s_last, n, acc, rsq, W, out, done, post, seq);
}
// statement blockIdx.y (gridDim.x blocks each): its accumulators at acc + y * s_acc words, its hand at W + y * s_w, its 16 sum
// words at out + 16 y and its block counter done[y]; the block of the statement that finishes last posts to slot y of the pinned
// batch mailbox (SCB256_SLOT_WORDS words per slot, laid out like the single call's post)
#define SCB256_SLOT_WORDS 32
__global__ __launch_bounds__(Z_THREADS) void partials256_batch_kernel(size_t n, u64* __restrict__ acc, size_t s_acc, E rsq, const E* __restrict__ W, size_t s_w,
                                                                      u64* __restrict__ out, u32* __restrict__ done, volatile u64* __restrict__ post, u64 seq) {
  __shared__ E sh[Z_THREADS];
  __shared__ u32 s_last;
  const size_t b = blockIdx.y;
  partials256_body(sh, &s_last, n, acc + b * s_acc, rsq, W + b * s_w, out + 16 * b, done + b, post + b * SCB256_SLOT_WORDS, seq);
}

// out[i] = in[2i] + r (in[2i+1] - in[2i]); tail: in (1 - r)   (dense.h:70-87, affine.h:26-52)
__device__ __forceinline__ void dense_bind256(size_t i, size_t n0, const E& r, const E* __restrict__ in, E* __restrict__ out) {
  if (i >= (n0 + 1) / 2) return;
  const E f0 = ld32(&in[2 * i]);
  E v;
  if (2 * i + 1 < n0) v = fp256_add(f0, fp256_mul(fp256_sub(ld32(&in[2 * i + 1]), f0), r));
  else v = fp256_sub(f0, fp256_mul(f0, r));
  st32(&out[i], v);
}

// HQuad::bind_h as an order-preserving compaction (see sumcheck.hip): a term is the second half of a merged pair iff its
// predecessor has the same other-hand corner and the even index h - 1
__device__ __forceinline__ bool is_second256(const uint2* hc, size_t i, int hand) {
  if (i == 0) return false;
  const uint2 a = hc[i - 1], b = hc[i];
  const u32 ah = hand ? a.y : a.x, ao = hand ? a.x : a.y, bh = hand ? b.y : b.x, bo = hand ? b.x : b.y;
  return ao == bo && (ah >> 1) == (bh >> 1) && bh == ah + 1;
}
__global__ __launch_bounds__(Z_THREADS) void hquad_count256_kernel(size_t n, const uint2* __restrict__ hc, int hand, u32* __restrict__ block_counts) {
  __shared__ u32 cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * Z_THREADS + threadIdx.x;
  const bool head = i < n && !is_second256(hc, i, hand);
  const u64 mask = __ballot(head);
  if ((threadIdx.x & 63) == 0) atomicAdd(&cnt, (u32)__popcll(mask));
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = cnt;
}
__global__ __launch_bounds__(1024) void scan256_kernel(u32 nblocks, u32* __restrict__ block_counts, u32* __restrict__ total) {
  __shared__ u32 sh[1024];
  __shared__ u32 carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (u32 base = 0; base < nblocks; base += 1024) {
    const u32 i = base + threadIdx.x;
    const u32 v = i < nblocks ? block_counts[i] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (u32 off = 1; off < 1024; off <<= 1) {
      const u32 t = threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    const u32 incl = sh[threadIdx.x];
    if (i < nblocks) block_counts[i] = carry + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}
// block blk of HQuad::bind_h; WRITE_HC as in bindg_emit256_body.  Every thread of the block must call this.
template <bool WRITE_HC>
__device__ __forceinline__ void hquad_bind256_body(u32* wave_off, u32 blk, size_t n, const uint2* __restrict__ hc, const E* __restrict__ vc, const E& r, int hand,
                                                   const u32* __restrict__ block_off, uint2* __restrict__ hc_out, E* __restrict__ vc_out) {
  const size_t i = (size_t)blk * Z_THREADS + threadIdx.x;
  const bool head = i < n && !is_second256(hc, i, hand);
  const u64 mask = __ballot(head);
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_off[wave] = (u32)__popcll(mask);
  __syncthreads();
  u32 off = block_off[blk];
  for (u32 w = 0; w < wave; ++w) off += wave_off[w];
  off += (u32)__popcll(mask & ((1ull << lane) - 1));
  if (!head) return;
  uint2 h = hc[i];
  const u32 hh = hand ? h.y : h.x;
  const E v0 = ld32(&vc[i]);
  E v;
  if (i + 1 < n && is_second256(hc, i + 1, hand)) v = fp256_add(v0, fp256_mul(fp256_sub(ld32(&vc[i + 1]), v0), r));  // affine_interpolation
  else if ((hh & 1) == 0) v = fp256_sub(v0, fp256_mul(v0, r));                                                         // ..._nz_z
  else v = fp256_mul(v0, r);                                                                                            // ..._z_nz
  if (hand) h.y = hh >> 1;
  else h.x = hh >> 1;
  if (WRITE_HC) hc_out[off] = h;
  st32(&vc_out[off], v);
}
// Dense::bind of the hand that just received its challenge (blocks [0, nbd)) and HQuad::bind_h (the blocks after them) in
// one launch
__global__ __launch_bounds__(Z_THREADS) void bind256_kernel(u32 nbd, size_t n0, const E* __restrict__ win, E* __restrict__ wout, size_t n,
                                                            const uint2* __restrict__ hc, const E* __restrict__ vc, E r, int hand,
                                                            const u32* __restrict__ block_off, uint2* __restrict__ hc_out, E* __restrict__ vc_out) {
  __shared__ u32 wave_off[Z_THREADS / 64];
  if (blockIdx.x < nbd) {
    dense_bind256((size_t)blockIdx.x * Z_THREADS + threadIdx.x, n0, r, win, wout);
    return;
  }
  hquad_bind256_body<true>(wave_off, blockIdx.x - nbd, n, hc, vc, r, hand, block_off, hc_out, vc_out);
}
// statement blockIdx.y with its challenge ch.r[y] (kernel arguments: 2 KiB at LFGPU_SC_BATCH_MAX statements): its hand at
// win + y * s_in -> wout + y * s_out, its HQUAD values at vc + y * s_vc -> vc_out + y * s_vc; the corners and the recorded
// offsets are shared, statement 0 writes the bound corners
struct Chal256 {
  E r[LFGPU_SC_BATCH_MAX];
};
__global__ __launch_bounds__(Z_THREADS) void bind256_batch_kernel(u32 nbd, size_t n0, const E* __restrict__ win, size_t s_in, E* __restrict__ wout, size_t s_out,
                                                                  size_t n, const uint2* __restrict__ hc, const E* __restrict__ vc, size_t s_vc, Chal256 ch, int hand,
                                                                  const u32* __restrict__ block_off, uint2* __restrict__ hc_out, E* __restrict__ vc_out) {
  __shared__ u32 wave_off[Z_THREADS / 64];
  const size_t b = blockIdx.y;
  const E r = ch.r[b];
  if (blockIdx.x < nbd) {
    dense_bind256((size_t)blockIdx.x * Z_THREADS + threadIdx.x, n0, r, win + b * s_in, wout + b * s_out);
    return;
  }
  if (b == 0) hquad_bind256_body<true>(wave_off, blockIdx.x - nbd, n, hc, vc, r, hand, block_off, hc_out, vc_out);
  else hquad_bind256_body<false>(wave_off, blockIdx.x - nbd, n, hc, vc + b * s_vc, r, hand, block_off, hc_out, vc_out + b * s_vc);
}

// ---- one round-hand of a batch in ONE launch once the HQUAD and both hand arrays have <= SCB256_SMALL_MAX entries: workgroup
// y = statement y does the pending Dense::bind + HQuad::bind_h with the previous challenge, the QW scatter, the two sums and its
// post, with block barriers between the phases.  The scatter's limb accumulators and the bound corners stay in LDS from one
// phase to the next; the bound values and hand array go to the statement's device arrays, which the next step starts from.
// The bound: LDS holds 64 bytes of accumulators and 8 bytes of corners per entry next to the 8 KiB of the block sum, and a
// workgroup may take 160 KiB: 72 N + 8 KiB <= 160 KiB gives N <= 2161, and 2048 is the largest power of two below that.
// The arithmetic is the bodies above, block by block, so every statement gets the bytes of the three-launch path.
#define SCB256_SMALL_MAX LFGPU_P256_BATCH_SMALL_MAX  // 2048 (lfgpu.h)
static_assert(SCB256_SMALL_MAX * 72 + Z_THREADS * 32 + 64 <= 160 * 1024, "the fused step's LDS: accumulators, corners, block sum");
#define SCB256_SMALL_LDS ((size_t)SCB256_SMALL_MAX * 72)
struct Small256 {
  int do_bind, bind_hand, do_eval, eval_hand;
  const uint2* hc_in;  // shared corners before the bind
  uint2* hc_out;       // ... after it (statement 0 writes them)
  const E* vc_in;      // HQUAD values, statement y at + y * s_vc
  E* vc_out;
  size_t s_vc;
  u32 nh, nh_out;  // HQUAD size before / after the bind (host-known: a circuit constant)
  const E* W[2];   // hand arrays before the bind, statement y at + y * s_W[h]
  size_t s_W[2];
  u32 nW[2];
  E* Wdst;  // destination of the dense bind, statement y at + y * s_Wdst
  size_t s_Wdst;
  const u32* block_off;  // the recorded offsets of the bind's round-hand
  E rsq;
};
__global__ __launch_bounds__(Z_THREADS) void sc_small_step_batch256_kernel(Small256 a, Chal256 ch, volatile u64* __restrict__ post, u64 seq) {
  extern __shared__ __attribute__((aligned(16))) u64 s_dyn[];
  __shared__ E sh[Z_THREADS];
  __shared__ u32 wave_off[Z_THREADS / 64];
  u64* qw = s_dyn;                                       // 8 words per target
  uint2* s_hc = (uint2*)(s_dyn + 8 * SCB256_SMALL_MAX);  // the corners after the bind
  const size_t b = blockIdx.x;
  const uint2* hc = a.hc_in;
  const E* vc = a.vc_in + b * a.s_vc;
  u32 nh = a.nh;
  const E* W[2] = {a.W[0] + b * a.s_W[0], a.W[1] + b * a.s_W[1]};
  u32 nW[2] = {a.nW[0], a.nW[1]};
  if (a.do_bind) {
    const E r = ch.r[b];
    const int h = a.bind_hand;
    E* dst = a.Wdst + b * a.s_Wdst;
    E* vco = a.vc_out + b * a.s_vc;
    for (u32 blk = 0; (size_t)blk * Z_THREADS < (nW[h] + 1) / 2; ++blk) dense_bind256((size_t)blk * Z_THREADS + threadIdx.x, nW[h], r, W[h], dst);
    for (u32 blk = 0; (size_t)blk * Z_THREADS < nh; ++blk) {  // block-uniform trip count: the body holds a barrier
      hquad_bind256_body<true>(wave_off, blk, nh, hc, vc, r, h, a.block_off, s_hc, vco);
      __syncthreads();  // wave_off is free again; after the last block: everything bound is visible to the workgroup
    }
    __threadfence_block();
    __syncthreads();
    nh = nh ? a.nh_out : 0;
    if (b == 0)
      for (u32 i = threadIdx.x; i < nh; i += Z_THREADS) a.hc_out[i] = s_hc[i];
    hc = s_hc;
    vc = vco;
    W[h] = dst;
    nW[h] = (nW[h] + 1) / 2;
  }
  if (!a.do_eval) return;
  const int h = a.eval_hand;
  for (u32 i = threadIdx.x; i < 8 * nW[h]; i += Z_THREADS) qw[i] = 0;
  __syncthreads();
  for (u32 blk = 0; (size_t)blk * Z_THREADS < nh; ++blk) qw_scatter256_body(blk, nh, hc, vc, h, W[1 - h], qw);
  __syncthreads();
  E a0 = e32_zero(), a2 = e32_zero();
  partials256_thread(0, 1, nW[h], qw, a.rsq, W[h], a0, a2);
  a0 = block_sum256(a0, sh);
  a2 = block_sum256(a2, sh);
  if (threadIdx.x < 64) {  // the sums as the 16 limb words the three-launch path posts; lane 0 then publishes
    volatile u64* slot = post + b * SCB256_SLOT_WORDS;
    if (threadIdx.x < 16) {
      u64 l = 0;
#pragma unroll
      for (u32 k = 0; k < 4; ++k)
        if (((threadIdx.x & 7) >> 1) == k) l = threadIdx.x < 8 ? a0.l[k] : a2.l[k];
      slot[threadIdx.x] = (threadIdx.x & 1) ? l >> 32 : (u64)(u32)l;
      __threadfence_system();
    }
    if (threadIdx.x == 0) __hip_atomic_store((u64*)&slot[16], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// out[3 y + 0 / 1 / 2] = statement y's W[0][0], W[1][0] and HQUAD scalar at the end of a layer
__global__ __launch_bounds__(Z_THREADS) void readout256_batch_kernel(u32 nb, const E* __restrict__ W0, size_t s0, const E* __restrict__ W1, size_t s1,
                                                                     const E* __restrict__ vc, size_t s_vc, E* __restrict__ out) {
  const u32 t = threadIdx.x;
  if (t >= 3 * nb) return;
  const size_t b = t / 3;
  const u32 k = t % 3;
  st32(&out[t], ld32(k == 0 ? &W0[b * s0] : k == 1 ? &W1[b * s1] : &vc[b * s_vc]));
}

// ---- the rest of a layer in ONE launch of co-resident workgroups (what sc_grid_layer_kernel is for the 16-byte fields,
// sumcheck.hip: same phases, same bounded waits, without its LDS tail and wave-split variants).  Per round-hand:
//   barrier | sums a0, a2 -> per-workgroup slots -> the workgroup that arrives last folds them and posts to the host |
//   layout of HQuad::bind_h (which entries merge, where each result goes: nothing of it needs the challenge, so it hides behind
//   the host's turn) | challenge (eight tagged words) | Dense::bind + HQUAD values + the NEXT evaluation's accumulators from
//   those values (double-buffered) | workgroups beyond ceil(largest array / per_wg) leave.
// Launched as an ordinary kernel of <= G256_WGS <= #CU workgroups (the host checks co-residency); every wait is bounded by an
// abort flag and a wall-clock timeout, so all waves always leave.
#define G256_THREADS 512
#define G256_WGS 128
#define G256_MAX (128u * 1024u)  // largest HQUAD / hand array the grid takes
struct Grid256Sync {  // device memory, zeroed before every launch
  u32 count, gen, abort, arrive;
  u64 chal[8];  // the challenge as the host's eight tagged words
  u64 pad_[6];
  u32 l1_bar[8 * 16];  // first-level arrival counters of the barrier, one cache line each
  u32 l1_arr[8 * 16];  // ... of the sums' arrival ticket
  u64 slots[8 * G256_WGS];  // per workgroup {a0, a2}
};
struct Grid256 {
  uint2* hcA;  // current HQUAD
  E* vcA;
  uint2* hcB;  // the other half of the ping-pong
  E* vcB;
  u32 nh;
  const E* W[2];  // hand arrays at entry
  u32 nW[2];
  E* Wb[2][2];  // bind destinations per hand (ping-pong)
  u64* QW;      // limb accumulators of the evaluation being summed, 8 words per target
  u64* QW2;     // of the next one
  u32 rh0, rh1;  // round-hands [rh0, rh1), rh1 = 2 logw
  u64 seq0, timeout_ticks;
  volatile u64* post;
  const volatile u64* cmd;
  Grid256Sync* gs;
  u32* counts;  // one word per workgroup
  u32* src;     // one word per HQUAD entry: where each bound entry comes from (+ its merge kind in the top bits)
  u32 per_wg;
  u32 wave_tail;  // 1: once everything fits 64 entries, ONE wave finishes the layer
  u32 test_drop;  // test only: the last workgroup leaves at once, as if it had never been placed
  u64 place_ticks;  // how long the FIRST barrier waits: the check that all workgroups were placed together
  E rsq;
};
// two-level arrival ticket (see sc_arrive in sumcheck.hip): true for the one workgroup that arrives last
__device__ __forceinline__ bool g256_arrive(u32* lvl1, u32* lvl2, u32 G, u32 g) {
  const u32 grp = g & 7, ngrp = G < 8 ? G : 8, members = (G - grp + 7) >> 3;
  u32* c1 = lvl1 + grp * 16;
  if (__hip_atomic_fetch_add(c1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != members - 1) return false;
  __hip_atomic_store(c1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (__hip_atomic_fetch_add(lvl2, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != ngrp - 1) return false;
  __hip_atomic_store(lvl2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}
// barrier among the first G workgroups, waiting at most limit_ticks; 0 = passed, 1 = aborted by another workgroup, 2 = this
// workgroup's wait ran out and it raised the abort flag first (every caller returns on non-zero)
__device__ __forceinline__ int g256_barrier_ex(Grid256Sync* gs, u32 G, u32& gen, u64 limit_ticks) {
  __shared__ u32 s_abort;
  if (G == 1) {
    __threadfence_block();
    __syncthreads();
    return 0;
  }
  // every storing wave: its stores are acknowledged before thread 0 releases for them (as in sc_grid_barrier_ex, sumcheck.hip)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 ab = 0;
    const u64 t0 = wall_clock64();
    if (g256_arrive(gs->l1_bar, &gs->count, G, blockIdx.x)) {
      // a workgroup that was placed only after the others gave up arrives last: it must not open the barrier for itself
      if (__hip_atomic_load(&gs->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ab = 1;
      else __hip_atomic_fetch_add(&gs->gen, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      while (__hip_atomic_load(&gs->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen) {
        if (__hip_atomic_load(&gs->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
          ab = 1;
          break;
        }
        if (wall_clock64() - t0 > limit_ticks) {  // never reached in a healthy run: no wait is unbounded
          ab = __hip_atomic_exchange(&gs->abort, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0 ? 2u : 1u;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    s_abort = ab;
  }
  ++gen;
  __syncthreads();
  return (int)s_abort;
}
__device__ __forceinline__ bool g256_barrier(Grid256Sync* gs, u32 G, u32& gen, u64 timeout_ticks) {
  return g256_barrier_ex(gs, G, gen, 2 * timeout_ticks) == 0;
}

__global__ __launch_bounds__(G256_THREADS) void grid256_layer_kernel(Grid256 a) {
  __shared__ E s_red[2][G256_THREADS / 64];
  __shared__ u32 s_wave[G256_THREADS / 64];
  __shared__ u32 s_carry, s_off, s_tot, s_last;
  __shared__ u64 s_cmd[5];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 g = blockIdx.x;
  u32 G = gridDim.x;  // active workgroups: shrinks with the data
  Grid256Sync* gs = a.gs;
  const uint2* hc = a.hcA;
  const E* vc = a.vcA;
  uint2* hc_o = a.hcB;
  E* vc_o = a.vcB;
  u32 nh = a.nh;
  const E* W[2] = {a.W[0], a.W[1]};
  u32 nW[2] = {a.nW[0], a.nW[1]};
  u32 wsel[2] = {a.W[0] == a.Wb[0][0] ? 1u : 0u, a.W[1] == a.Wb[1][0] ? 1u : 0u};
  u64* QW = a.QW;
  u64* QWn = a.QW2;
  u32 gen = 0;
  u64 seq = a.seq0;
  bool wave_mode = false;
  __shared__ uint2 t_hc[2][64];  // the state of the single-wave tail (<= 64 entries per array)
  __shared__ E t_vc[2][64];
  __shared__ E t_w[2][128];      // per hand: current (64) + two bind destinations (32 each)
  __shared__ u64 t_qw[2][8 * 64];
  __shared__ u32 t_src[64];
  E* Wd[2][2] = {{a.Wb[0][0], a.Wb[0][1]}, {a.Wb[1][0], a.Wb[1][1]}};
  u32* srcp = a.src;
  const E rsq = a.rsq;
  {
    const u32 GT = G * G256_THREADS, gtid = (wave * G + g) * 64 + lane;  // 64-entry chunks dealt round-robin over the workgroups
    const u32 h0 = a.rh0 & 1;
    for (u32 i = gtid; i < 8 * nW[h0]; i += GT) QW[i] = 0;
    for (u32 i = gtid; i < 8 * nW[1 - h0]; i += GT) QWn[i] = 0;
  }
  // placement check (see sc_grid_layer_kernel, sumcheck.hip): only scratch has been written so far; when not every workgroup
  // shows up, the one whose wait runs out first reports status 2 and the host continues with per-launch kernels
  if (a.test_drop && G > 1 && g == G - 1) return;
  {
    const int br = g256_barrier_ex(gs, G, gen, a.place_ticks);
    if (br) {
      if (br == 2 && tid == 0) {
        a.post[9] = 2;
        __threadfence_system();
        __hip_atomic_store((u64*)&a.post[16], a.seq0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      return;
    }
  }
  {  // first evaluation of the hand-off: QW[h[hand]] += v * Wother[h[1-hand]] over the whole HQUAD
    const int hand = (int)(a.rh0 & 1);
    const u32 GT = G * G256_THREADS;
    const E* Wo = W[1 - hand];
    for (u32 base = (wave * G + g) * 64; base < (nh + 63) / 64 * 64; base += GT) {  // whole waves: the fold shuffles
      const u32 i = base + lane;
      u32 key = 0xffffffffu;
      E t = e32_zero();
      if (i < nh) {
        const uint2 h = hc[i];
        key = hand ? h.y : h.x;
        t = fp256_mul(ld32(&vc[i]), ld32(&Wo[hand ? h.x : h.y]));
      }
      run_fold_commit256(key, t, QW);
    }
  }
  for (u32 rh = a.rh0; rh < a.rh1; ++rh, ++seq) {
    const int hand = (int)(rh & 1);
    if (!g256_barrier(gs, G, gen, a.timeout_ticks)) return;  // the accumulators of this evaluation are complete
    {  // shrink: one workgroup per per_wg entries of the largest array; the others are done
      u32 big = nh > nW[0] ? nh : nW[0];
      big = big > nW[1] ? big : nW[1];
      u32 want = (big + a.per_wg - 1) / a.per_wg;
      want = want ? want : 1;
      if (want < G) G = want;
      if (g >= G) return;
    }
    // ---- the last rounds of a layer: at most 64 entries in every array.  Wave 0 finishes the layer alone (see the same
    // block of sc_grid_layer_kernel, sumcheck.hip): both sums in ONE product (lanes 0-31 the a0 terms, lanes 32-63 the a2
    // terms), both binds in one product when they fit the wave together, the layout by ballot, the sums by shuffles; no
    // workgroup barrier is left -- the other waves have ended.  Same field operations on the same operands as below.
    if (G == 1 && a.wave_tail && !wave_mode && nh <= 64 && nW[0] <= 64 && nW[1] <= 64) {
      if (wave != 0) return;  // the barrier at the top of the loop was their last one: everything they wrote is visible
      wave_mode = true;
      // the whole state moves into LDS (21 KiB): every phase is then a product plus an LDS round trip instead of a product
      // plus one or two trips to L2
      if (lane < nh) {
        t_hc[0][lane] = hc[lane];
        st32(&t_vc[0][lane], ld32(&vc[lane]));
      }
      for (int h = 0; h < 2; ++h)
        if (lane < nW[h]) st32(&t_w[h][lane], ld32(&W[h][lane]));
      for (u32 i = lane; i < 8 * 64; i += 64) {
        t_qw[0][i] = i < 8 * nW[hand] ? QW[i] : 0;  // the sums of this evaluation
        t_qw[1][i] = 0;
      }
      hc = t_hc[0]; hc_o = t_hc[1]; vc = t_vc[0]; vc_o = t_vc[1];
      for (int h = 0; h < 2; ++h) {
        W[h] = t_w[h];
        Wd[h][0] = t_w[h] + 64;
        Wd[h][1] = t_w[h] + 96;
        wsel[h] = 0;
      }
      QW = t_qw[0];
      QWn = t_qw[1];
      srcp = t_src;
      __threadfence_block();
      __syncthreads();
    }
    if (wave_mode) {
      const u32 nq = nW[hand], nodd = nq / 2;
      const E* Wh = W[hand];
      auto qw_at = [&](u32 j) -> E {
        u64 q[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = QW[8 * (size_t)j + k];
        return fp256_reduce_limbs(q, rsq);
      };
      E x = e32_zero(), y = e32_zero();
      {
        const u32 i = lane & 31;
        if (i < nodd) {
          const E q0 = qw_at(2 * i), w0 = ld32(&Wh[2 * i]);
          if (lane < 32) {
            x = q0;
            y = w0;
          } else {
            x = fp256_sub(qw_at(2 * i + 1), q0);
            y = fp256_sub(ld32(&Wh[2 * i + 1]), w0);
          }
        } else if (i == nodd && 2 * nodd < nq) {  // odd tail (prover_layers.h:381-388): in both sums
          x = qw_at(2 * nodd);
          y = ld32(&Wh[2 * nodd]);
        }
      }
      E t = fp256_mul(x, y);
      for (int off = 16; off > 0; off >>= 1) {  // sums inside each half of the wave
        E o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o.l[k] = __shfl_down(t.l[k], off, 32);
        t = fp256_add(t, o);
      }
      E a2;
#pragma unroll
      for (int k = 0; k < 4; ++k) a2.l[k] = __shfl(t.l[k], 32, 64);
      if (lane == 0) {
        u64* po = (u64*)a.post;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          __hip_atomic_store(&po[k], t.l[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(&po[4 + k], a2.l[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __hip_atomic_store(&po[8], (u64)nh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&po[9], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        lf_wait_stores_before_publish();  // payload acknowledged before the sequence word leaves
        __hip_atomic_store(&po[16], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      // layout of HQuad::bind_h (no challenge needed): lane i looks at entry i
      const bool head = lane < nh && !is_second256(hc, lane, hand);
      const u64 hmask = __ballot(head);
      const u32 new_nh = (u32)__popcll(hmask);
      if (head) {
        const u32 off = (u32)__popcll(hmask & ((1ull << lane) - 1));
        uint2 h = hc[lane];
        const u32 hh = hand ? h.y : h.x;
        const u32 kind = (lane + 1 < nh && is_second256(hc, lane + 1, hand)) ? 0u : ((hh & 1) == 0 ? 1u : 2u);
        if (hand) h.y = hh >> 1;
        else h.x = hh >> 1;
        hc_o[off] = h;
        srcp[off] = lane | (kind << 30);
      }
      // the challenge: eight tagged words (see below)
      u64 w = 0;
      {
        const u64 t0 = wall_clock64();
        const u64 tag = seq & 0xffffffffull;
        for (;;) {
          if (lane < 8) w = __hip_atomic_load((const u64*)&a.cmd[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          if (__all(lane >= 8 || (w >> 32) == tag)) break;
          int stop = 0;
          if (lane == 0 && wall_clock64() - t0 > a.timeout_ticks) {  // the host went away: report and leave
            a.post[9] = 1;
            __threadfence_system();
            __hip_atomic_store((u64*)&a.post[16], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            stop = 1;
          }
          if (__shfl(stop, 0, 64)) return;
          __builtin_amdgcn_s_sleep(1);
        }
      }
      E r;
      {
        const u64 lo32 = w & 0xffffffffull;
#pragma unroll
        for (int k = 0; k < 4; ++k) r.l[k] = __shfl(lo32, 2 * k, 64) | (__shfl(lo32, 2 * k + 1, 64) << 32);
      }
      const E* Wold = W[hand];
      const u32 n0 = nW[hand], nout = (n0 + 1) / 2;
      for (u32 i = lane; i < 8 * nout; i += 64) QW[i] = 0;  // next written two round-hands from now, for this hand again
      __threadfence_block();
      __syncthreads();  // one wave: a wait for the stores above (layout, clear)
      // Dense::bind of W[hand] and the HQuad::bind_h values: out = base + d * r for both (hquad.h:94-118)
      E* const Wout = Wd[hand][wsel[hand]];
      const bool merged = new_nh + nout <= 64;  // both binds in one pass: HQUAD values on the low lanes, the hand array on the high ones
      E vbound = e32_zero();
      for (int pass = 0; pass < (merged ? 1 : 2); ++pass) {
        E base = e32_zero(), d = e32_zero();
        int job = 0;  // 1: HQUAD value `lane`, 2: hand entry j
        u32 j = 0;
        if (pass == 0 && lane < new_nh) {
          job = 1;
          const u32 sidx = srcp[lane], i = sidx & 0x3fffffffu, kind = sidx >> 30;
          const E v0 = ld32(&vc[i]);
          if (kind == 0) {
            base = v0;
            d = fp256_sub(ld32(&vc[i + 1]), v0);
          } else if (kind == 1) {
            base = v0;
            d = fp256_sub(e32_zero(), v0);
          } else {
            d = v0;
          }
        } else if (merged ? lane >= 64 - nout : (pass == 1 && lane < nout)) {
          job = 2;
          j = merged ? lane - (64 - nout) : lane;
          const E f0 = ld32(&Wold[2 * j]);
          base = f0;
          d = 2 * j + 1 < n0 ? fp256_sub(ld32(&Wold[2 * j + 1]), f0) : fp256_sub(e32_zero(), f0);
        }
        const E out = fp256_add(base, fp256_mul(d, r));
        if (job == 1) {
          vbound = out;
          st32(&vc_o[lane], out);
        } else if (job == 2) {
          st32(&Wout[j], out);
        }
      }
      __threadfence_block();
      __syncthreads();
      if (rh + 1 < a.rh1) {  // the next evaluation's accumulators (for the other hand)
        u32 key = 0xffffffffu;
        E tt = e32_zero();
        if (lane < new_nh) {
          const uint2 h = hc_o[lane];
          key = hand ? h.x : h.y;
          tt = fp256_mul(vbound, ld32(&Wout[hand ? h.y : h.x]));
        }
        run_fold_commit256(key, tt, QWn);
      }
      W[hand] = Wout;
      nW[hand] = nout;
      wsel[hand] ^= 1;
      {
        nh = new_nh;
        uint2* th = const_cast<uint2*>(hc);
        E* tv = const_cast<E*>(vc);
        hc = hc_o;
        vc = vc_o;
        hc_o = th;
        vc_o = tv;
        u64* tq = QW;
        QW = QWn;
        QWn = tq;
      }
      continue;
    }
    const u32 GT = G * G256_THREADS, gtid = (wave * G + g) * 64 + lane;
    // ---- ProverLayers::evaluations: a0, a2 from the accumulators
    {
      const u32 nq = nW[hand], nodd = nq / 2;
      const E* Wh = W[hand];
      auto qw_at = [&](u32 j) -> E {
        u64 q[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = QW[8 * (size_t)j + k];
        return fp256_reduce_limbs(q, rsq);
      };
      E a0 = e32_zero(), a2 = e32_zero();
      if (G == 1) {  // one workgroup left: the two products of a pair on different waves (even waves sum a0, odd waves a2)
        const u32 half = G256_THREADS / 2, ht = (wave >> 1) * 64 + lane;
        const bool second = (wave & 1) != 0;
        for (u32 i = ht; i < nodd; i += half) {
          const E q0 = qw_at(2 * i), w0 = ld32(&Wh[2 * i]);
          if (!second) a0 = fp256_add(a0, fp256_mul(q0, w0));
          else a2 = fp256_add(a2, fp256_mul(fp256_sub(qw_at(2 * i + 1), q0), fp256_sub(ld32(&Wh[2 * i + 1]), w0)));
        }
        if (ht == 0 && 2 * nodd < nq) {  // odd tail (prover_layers.h:381-388): in both sums
          const E t = fp256_mul(qw_at(2 * nodd), ld32(&Wh[2 * nodd]));
          if (!second) a0 = fp256_add(a0, t);
          else a2 = fp256_add(a2, t);
        }
      } else {
        for (u32 i = gtid; i < nodd; i += GT) {
          const E q0 = qw_at(2 * i), q1 = qw_at(2 * i + 1), w0 = ld32(&Wh[2 * i]), w1 = ld32(&Wh[2 * i + 1]);
          a0 = fp256_add(a0, fp256_mul(q0, w0));
          a2 = fp256_add(a2, fp256_mul(fp256_sub(q1, q0), fp256_sub(w1, w0)));
        }
        if (gtid == 0 && 2 * nodd < nq) {  // odd tail (prover_layers.h:381-388)
          const E t = fp256_mul(qw_at(2 * nodd), ld32(&Wh[2 * nodd]));
          a0 = fp256_add(a0, t);
          a2 = fp256_add(a2, t);
        }
      }
      auto wg_sum = [&](E& x0, E& x2, bool split) {  // wave shuffles, then the wave sums through LDS; result in thread 0
        if (split) {  // even waves carry only a0, odd waves only a2: one value to fold per wave
          const bool second = (wave & 1) != 0;
          E v = second ? x2 : x0;
          for (int off = 32; off > 0; off >>= 1) {
            E o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o.l[k] = __shfl_down(v.l[k], off, 64);
            v = fp256_add(v, o);
          }
          x0 = second ? e32_zero() : v;
          x2 = second ? v : e32_zero();
        } else {
          for (int off = 32; off > 0; off >>= 1) {
            E o0, o2;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              o0.l[k] = __shfl_down(x0.l[k], off, 64);
              o2.l[k] = __shfl_down(x2.l[k], off, 64);
            }
            x0 = fp256_add(x0, o0);
            x2 = fp256_add(x2, o2);
          }
        }
        if (lane == 0) {
          s_red[0][wave] = x0;
          s_red[1][wave] = x2;
        }
        __syncthreads();
        if (wave == 0) {  // the 8 wave sums of a0 on lanes 0-7, of a2 on lanes 8-15: three shuffle steps instead of 14 additions in a row
          E v = lane < 16 ? s_red[lane >> 3][lane & 7] : e32_zero();
#pragma unroll
          for (int off = 4; off > 0; off >>= 1) {
            E o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o.l[k] = __shfl_down(v.l[k], off, 64);
            v = fp256_add(v, o);
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            x0.l[k] = __shfl(v.l[k], 0, 64);
            x2.l[k] = __shfl(v.l[k], 8, 64);
          }
        }
        __syncthreads();
      };
      wg_sum(a0, a2, G == 1);
      bool poster = tid == 0;
      if (G > 1) {  // slots + arrival ticket: the last workgroup to arrive folds all slots
        if (tid == 0) {
          u64* sl = &gs->slots[8 * g];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            sl[k] = a0.l[k];
            sl[4 + k] = a2.l[k];
          }
          s_last = g256_arrive(gs->l1_arr, &gs->arrive, G, g) ? 1u : 0u;  // releases the slot
        }
        __syncthreads();
        poster = false;
        if (s_last) {  // uniform per workgroup
          a0 = e32_zero();
          a2 = e32_zero();
          if (tid < G) {
            const u64* sl = &gs->slots[8 * tid];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              a0.l[k] = __hip_atomic_load(&sl[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              a2.l[k] = __hip_atomic_load(&sl[4 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
          wg_sum(a0, a2, false);
          poster = tid == 0;
        }
      }
      if (poster) {  // system-scope stores into the pinned words, then the sequence number
        u64* po = (u64*)a.post;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          __hip_atomic_store(&po[k], a0.l[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(&po[4 + k], a2.l[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __hip_atomic_store(&po[8], (u64)nh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&po[9], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        lf_wait_stores_before_publish();  // payload acknowledged before the sequence word leaves
        __hip_atomic_store(&po[16], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    // ---- while the host works on the challenge: the layout of HQuad::bind_h
    u32 my_off, my_end, new_nh;
    {
      const u32 R = ((nh + G - 1) / G + 63) / 64 * 64;  // range per workgroup, whole waves
      const u32 lo = (u64)g * R < nh ? g * R : nh, hi = (u64)lo + R < nh ? lo + R : nh;
      if (tid == 0) {
        s_carry = 0;
        s_off = 0;
        s_tot = 0;
      }
      __syncthreads();
      if (G > 1) {
        u32 mine = 0;
        for (u32 base = lo; base < hi; base += G256_THREADS) {
          const u32 i = base + tid;
          const bool head = i < hi && !is_second256(hc, i, hand);
          mine += (u32)__popcll(__ballot(head));
        }
        if (lane == 0 && mine) atomicAdd(&s_carry, mine);
        __syncthreads();
        if (tid == 0) a.counts[g] = s_carry;
        if (!g256_barrier(gs, G, gen, a.timeout_ticks)) return;
        if (tid < G) {
          const u32 cnt = a.counts[tid];
          if (cnt) {
            atomicAdd(&s_tot, cnt);
            if (tid < g) atomicAdd(&s_off, cnt);
          }
        }
        __syncthreads();
      }
      my_off = s_off;
      __syncthreads();
      if (tid == 0) s_carry = my_off;
      __syncthreads();
      for (u32 base = lo; base < hi; base += G256_THREADS) {
        const u32 i = base + tid;
        const bool head = i < hi && !is_second256(hc, i, hand);
        const u64 mask = __ballot(head);
        if (lane == 0) s_wave[wave] = (u32)__popcll(mask);
        __syncthreads();
        u32 off = s_carry;
        for (u32 w = 0; w < wave; ++w) off += s_wave[w];
        off += (u32)__popcll(mask & ((1ull << lane) - 1));
        if (head) {
          uint2 h = hc[i];
          const u32 hh = hand ? h.y : h.x;
          const u32 kind = (i + 1 < nh && is_second256(hc, i + 1, hand)) ? 0u : ((hh & 1) == 0 ? 1u : 2u);
          if (hand) h.y = hh >> 1;
          else h.x = hh >> 1;
          hc_o[off] = h;
          a.src[off] = i | (kind << 30);
        }
        __syncthreads();
        if (tid == 0) {
          u32 tot = 0;
          for (u32 w = 0; w < G256_THREADS / 64; ++w) tot += s_wave[w];
          s_carry += tot;
        }
        __syncthreads();
      }
      my_end = s_carry;
      new_nh = G > 1 ? s_tot : my_end;
    }
    // ---- the challenge: eight 64-bit words {tag = low half of the sequence number, 32 bits of the challenge}; a read that
    // finds the tag in all eight has the whole challenge.  Workgroup 0 polls the host and hands it on through a device slot.
    if (wave == 0) {
      const u64 t0 = wall_clock64();
      const u64 tag = seq & 0xffffffffull;
      const bool from_host = g == 0;
      u64 got = 0, w = 0;
      for (;;) {
        if (lane < 8) {
          if (from_host) w = __hip_atomic_load((const u64*)&a.cmd[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          else w = __hip_atomic_load(&gs->chal[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (__all(lane >= 8 || (w >> 32) == tag)) {
          got = seq;
          break;
        }
        int stop = 0;
        if (lane == 0) {
          if (G > 1 && __hip_atomic_load(&gs->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) stop = 1;
          else if (wall_clock64() - t0 > (from_host ? 1 : 2) * a.timeout_ticks) {  // the host went away: release every workgroup and report
            __hip_atomic_store(&gs->abort, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            if (g == 0) {
              a.post[9] = 1;
              __threadfence_system();
              __hip_atomic_store((u64*)&a.post[16], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            stop = 1;
          }
        }
        if (__shfl(stop, 0, 64)) break;
        __builtin_amdgcn_s_sleep(1);
      }
      if (got == seq && g == 0 && G > 1 && lane < 8) __hip_atomic_store(&gs->chal[lane], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const u64 lo32 = w & 0xffffffffull;
      const u64 even = __shfl(lo32, (lane & 3) * 2, 64), odd = __shfl(lo32, (lane & 3) * 2 + 1, 64);
      if (lane < 4) s_cmd[lane] = even | (odd << 32);
      if (lane == 0) s_cmd[4] = got;
    }
    __syncthreads();
    if (s_cmd[4] != seq) return;  // uniform per workgroup; the barriers of the others see the abort flag
    E r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.l[k] = s_cmd[k];
    // ---- Dense::bind of W[hand] (out of place); the HQUAD values for the layout above; and, from those values, the next
    // evaluation's accumulators -- the bound hand entry is recomputed from the unbound array (one more product) so that no
    // workgroup waits for another one's Dense::bind
    const E* Wold = W[hand];
    const u32 n0 = nW[hand], nout = (n0 + 1) / 2;
    auto bind_at = [&](u32 j) -> E {
      const E f0 = ld32(&Wold[2 * j]);
      if (2 * j + 1 < n0) return fp256_add(f0, fp256_mul(fp256_sub(ld32(&Wold[2 * j + 1]), f0), r));
      return fp256_sub(f0, fp256_mul(f0, r));
    };
    const bool more = rh + 1 < a.rh1;
    for (u32 i = gtid; i < 8 * nout; i += GT) QW[i] = 0;  // next written two round-hands from now, for this hand again
    E* const Wout = a.Wb[hand][wsel[hand]];
    auto bind_value = [&](u32 o) -> E {  // HQuad::bind_h value of output o (hquad.h:94-118)
      const u32 sidx = a.src[o], i = sidx & 0x3fffffffu, kind = sidx >> 30;
      const E v0 = ld32(&vc[i]);
      if (kind == 0) return fp256_add(v0, fp256_mul(fp256_sub(ld32(&vc[i + 1]), v0), r));
      if (kind == 1) return fp256_sub(v0, fp256_mul(v0, r));
      return fp256_mul(v0, r);
    };
    if (G == 1) {
      // One workgroup left: what counts is the longest chain of instructions a single wave issues, so the independent products go
      // to different waves -- the even waves bind the HQUAD values while the odd waves bind the hand array -- and, a workgroup
      // barrier being cheap, the next evaluation's products take the bound hand entries from memory instead of recomputing them
      const u32 half = G256_THREADS / 2, ht = (wave >> 1) * 64 + lane;
      if ((wave & 1) == 0) {
        for (u32 o = ht; o < my_end; o += half) st32(&vc_o[o], bind_value(o));
      } else {
        for (u32 i = ht; i < nout; i += half) st32(&Wout[i], bind_at(i));
      }
      __threadfence_block();
      __syncthreads();
      if (more) {
        for (u32 base = 0; base < my_end; base += G256_THREADS) {
          const u32 o = base + tid;
          u32 key = 0xffffffffu;
          E t = e32_zero();
          if (o < my_end) {
            const uint2 h = hc_o[o];
            key = hand ? h.x : h.y;  // the next evaluation is for the other hand
            t = fp256_mul(ld32(&vc_o[o]), ld32(&Wout[hand ? h.y : h.x]));
          }
          run_fold_commit256(key, t, QWn);
        }
      }
    } else {
    for (u32 i = gtid; i < nout; i += GT) st32(&Wout[i], bind_at(i));
    for (u32 base = my_off; base < my_end; base += G256_THREADS) {
      const u32 o = base + tid;
      u32 key = 0xffffffffu;
      E t = e32_zero();
      if (o < my_end) {
        const u32 sidx = a.src[o], i = sidx & 0x3fffffffu, kind = sidx >> 30;
        const E v0 = ld32(&vc[i]);
        E v;
        if (kind == 0) v = fp256_add(v0, fp256_mul(fp256_sub(ld32(&vc[i + 1]), v0), r));  // HQuad::bind_h (hquad.h:94-118)
        else if (kind == 1) v = fp256_sub(v0, fp256_mul(v0, r));
        else v = fp256_mul(v0, r);
        st32(&vc_o[o], v);
        if (more) {
          const uint2 h = hc_o[o];
          key = hand ? h.x : h.y;  // the next evaluation is for the other hand
          t = fp256_mul(v, bind_at(hand ? h.y : h.x));
        }
      }
      if (more) run_fold_commit256(key, t, QWn);
    }
    }
    W[hand] = Wout;
    nW[hand] = nout;
    wsel[hand] ^= 1;
    {
      nh = new_nh;
      uint2* th = const_cast<uint2*>(hc);
      E* tv = const_cast<E*>(vc);
      hc = hc_o;
      vc = vc_o;
      hc_o = th;
      vc_o = tv;
      u64* tq = QW;
      QW = QWn;
      QWn = tq;
    }
  }
  if (g == 0 && tid == 0) {  // end of the layer: W[R,C], W[L,C] and HQUAD->scalar() (the last binds of this workgroup: G == 1 by now)
    __threadfence();
    const E w0 = nW[0] ? ld32(&W[0][0]) : e32_zero(), w1 = nW[1] ? ld32(&W[1][0]) : e32_zero(), sc = nh ? ld32(&vc[0]) : e32_zero();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a.post[k] = w0.l[k];
      a.post[4 + k] = w1.l[k];
      a.post[12 + k] = sc.l[k];
    }
    a.post[8] = nh;
    a.post[9] = 0;
    __threadfence_system();
    __hip_atomic_store((u64*)&a.post[16], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- Ligero row combinations (ligero.hip / sumcheck.hip, over 32-byte elements).  Every kernel has a batch twin (lig::prove_batch /
// open_batch through L32): statement blockIdx.y.  The B tableaux are the provers' own buffers and the dense blocks the caller's,
// so their base pointers come as ONE by-value argument indexed by the (wave-uniform) statement -- scalar loads from the kernarg
// segment (LfBatchPtrs, ctx.h); what the call owns (the A rows, the challenge vectors, the y vectors, the gathered columns) stands
// at one stride per statement.  Tableau rows are given as element offsets into a statement's tableau (o_*).  A pair shares one
// body, so the arithmetic per entry is the same in the same order.
// y[j] = y0[j] + sum_i f_i[j] T[i][j] with f_i[j] = A[i][j] (VEC: dot_proof, Blas::vaxpy blas.h:71-78) or u[i] (low_degree_proof):
// 64 columns x 4 row slices per workgroup, folded through LDS.  y0 may be y itself (rows_axpy256_kernel), so neither is __restrict__.
template <bool VEC>
__device__ __forceinline__ void rows_combo256_body(u32 nrows, size_t n, const E* y0, const E* __restrict__ f, size_t ldf, const E* __restrict__ T, size_t ld, E* y,
                                                   E (*part)[64]) {
  const u32 col = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const size_t j = (size_t)blockIdx.x * 64 + col;
  E acc = e32_zero();
  if (j < n)
    for (u32 i = slice; i < nrows; i += 4) acc = fp256_add(acc, fp256_mul(ld32(&T[(size_t)i * ld + j]), ld32(VEC ? &f[(size_t)i * ldf + j] : &f[i])));
  part[slice][col] = acc;
  __syncthreads();
  if (slice == 0 && j < n) {
    acc = ld32(&y0[j]);
    for (u32 k = 0; k < 4; ++k) acc = fp256_add(acc, part[k][col]);
    st32(&y[j], acc);
  }
}
// y[j] += sum_i u[i] T[i][j]
__global__ __launch_bounds__(256) void rows_axpy256_kernel(u32 nrows, size_t n, E* __restrict__ y, const E* __restrict__ u, const E* __restrict__ T, size_t ld) {
  __shared__ E part[4][64];
  rows_combo256_body<false>(nrows, n, y, u, 0, T, ld, y, part);
}
// y[j] = T0[j] + sum_i A[i][j] T[i][j]
__global__ __launch_bounds__(256) void rows_vaxpy256_kernel(u32 nrows, size_t n, const E* __restrict__ T0, const E* __restrict__ A, size_t lda,
                                                            const E* __restrict__ T, size_t ld, E* __restrict__ y) {
  __shared__ E part[4][64];
  rows_combo256_body<true>(nrows, n, T0, A, lda, T, ld, y, part);
}
// dot proof: y_b[j] = T_b[idot][j] + sum_i A_b[i][j] T_b[iw + i][j], j < n = dblock
__global__ __launch_bounds__(256) void rows_vaxpy256_batch_kernel(u32 nrows, size_t n, LfBatchPtrs T, size_t ld, size_t o_dot, size_t o_w, const E* __restrict__ A,
                                                                  size_t s_A, size_t lda, E* __restrict__ y, size_t s_y) {
  __shared__ E part[4][64];
  const size_t b = blockIdx.y;
  const E* Tb = (const E*)T.p[b];
  rows_combo256_body<true>(nrows, n, Tb + o_dot, A + b * s_A, lda, Tb + o_w, ld, y + b * s_y, part);
}
// low-degree proof: y_b[j] = T_b[ildt][j] + sum_i u_b[i] T_b[iw + i][j], j < n = block (the single path copies the ILDT row into
// y first and rows_axpy256_kernel adds to it: the same sum in the same order); u_b at u + b * s_u
__global__ __launch_bounds__(256) void rows_axpy256_batch_kernel(u32 nrows, size_t n, LfBatchPtrs T, size_t ld, size_t o_ldt, size_t o_w, const E* __restrict__ u,
                                                                 size_t s_u, E* __restrict__ y, size_t s_y) {
  __shared__ E part[4][64];
  const size_t b = blockIdx.y;
  const E* Tb = (const E*)T.p[b];
  rows_combo256_body<false>(nrows, n, Tb + o_ldt, u + b * s_u, 0, Tb + o_w, ld, y + b * s_y, part);
}
// y[j] = Tq[j] + sum_i u[i] (z_i[j] - x_i[j] y_i[j])   (quadratic_proof :311-333)
__device__ __forceinline__ void quad_combo256_body(u32 nt, size_t n, const E* __restrict__ Tq, const E* __restrict__ u, const E* __restrict__ X, const E* __restrict__ Y,
                                                   const E* __restrict__ Zr, size_t ld, E* __restrict__ y) {
  const size_t j = (size_t)blockIdx.x * Z_THREADS + threadIdx.x;
  if (j >= n) return;
  E acc = ld32(&Tq[j]);
  for (u32 i = 0; i < nt; ++i) {
    const E t = fp256_sub(ld32(&Zr[(size_t)i * ld + j]), fp256_mul(ld32(&X[(size_t)i * ld + j]), ld32(&Y[(size_t)i * ld + j])));
    acc = fp256_add(acc, fp256_mul(ld32(&u[i]), t));
  }
  st32(&y[j], acc);
}
__global__ __launch_bounds__(Z_THREADS) void quad_combo256_kernel(u32 nt, size_t n, const E* __restrict__ Tq, const E* __restrict__ u, const E* __restrict__ X,
                                                                  const E* __restrict__ Y, const E* __restrict__ Zr, size_t ld, E* __restrict__ y) {
  quad_combo256_body(nt, n, Tq, u, X, Y, Zr, ld, y);
}
// statement blockIdx.y: row IQUAD (o_quad) and the triples' rows x | y | z, nt rows apart from o_x on, of its own tableau; u_b = u + b * s_u
__global__ __launch_bounds__(Z_THREADS) void quad_combo256_batch_kernel(u32 nt, size_t n, LfBatchPtrs T, size_t ld, size_t o_quad, size_t o_x, const E* __restrict__ u,
                                                                        size_t s_u, E* __restrict__ y, size_t s_y) {
  const size_t b = blockIdx.y;
  const E* Tb = (const E*)T.p[b];
  const E* X = Tb + o_x;
  const E* Y = X + (size_t)nt * ld;
  quad_combo256_body(nt, n, Tb + o_quad, u + b * s_u, X, Y, Y + (size_t)nt * ld, ld, y + b * s_y);
}
// rows[i][r + j] = scale * dense[i w + j]; then rows[pos(idx)] += val (inner_product_vector + layout_Aext, ligero_param.h:382-430).
// No bound on idx in the kernels: the host has checked every list against nwqrow * w (lig::a_rows, lig::prove_batch).
__device__ __forceinline__ void a_rows_sparse256_body(u32 r, u32 w, size_t ld, const u64* __restrict__ idx, const E* __restrict__ val, size_t o, size_t n,
                                                      E* __restrict__ rows) {  // entries [o, o + n) of the lists
  const size_t t = (size_t)blockIdx.x * Z_THREADS + threadIdx.x;
  if (t >= n) return;
  const u64 f = idx[o + t];
  E* dst = &rows[(f / w) * ld + r + f % w];
  st32(dst, fp256_add(ld32(dst), ld32(&val[o + t])));
}
__global__ __launch_bounds__(Z_THREADS) void a_rows_dense256_kernel(u32 r, u32 w, size_t ld, E scale, const E* __restrict__ dense, size_t n, E* __restrict__ rows) {
  const size_t t = (size_t)blockIdx.x * Z_THREADS + threadIdx.x;
  if (t >= n) return;
  const size_t i = t / w, j = t % w;
  st32(&rows[i * ld + r + j], fp256_mul(scale, ld32(&dense[t])));
}
__global__ __launch_bounds__(Z_THREADS) void a_rows_sparse256_kernel(u32 r, u32 w, size_t ld, const u64* __restrict__ idx, const E* __restrict__ val, size_t n,
                                                                     E* __restrict__ rows) {
  a_rows_sparse256_body(r, w, ld, idx, val, 0, n, rows);
}
// rows of statement b at rows + b * s_rows: dense_b is a per-statement pointer, scaled by scale[b].  (Written out: through a shared
// body both dense kernels need more SGPRs, profiles/ligero_slab/README.md.)
__global__ __launch_bounds__(Z_THREADS) void a_rows_dense256_batch_kernel(u32 r, u32 w, size_t ld, const E* __restrict__ scale, LfBatchPtrs dense, size_t n,
                                                                          E* __restrict__ rows, size_t s_rows) {
  const size_t t = (size_t)blockIdx.x * Z_THREADS + threadIdx.x;
  if (t >= n) return;
  const size_t b = blockIdx.y, i = t / w, j = t % w;
  const E* __restrict__ d = (const E*)dense.p[b];
  st32(&rows[b * s_rows + i * ld + r + j], fp256_mul(ld32(&scale[b]), ld32(&d[t])));
}
// ONE packed (idx, val) list for all statements, statement b's entries at [off[b], off[b + 1]) (ragged; a statement may have none)
__global__ __launch_bounds__(Z_THREADS) void a_rows_sparse256_batch_kernel(u32 r, u32 w, size_t ld, const u64* __restrict__ idx, const E* __restrict__ val,
                                                                           const u64* __restrict__ off, E* __restrict__ rows, size_t s_rows) {
  const size_t b = blockIdx.y, o = off[b];
  a_rows_sparse256_body(r, w, ld, idx, val, o, off[b + 1] - o, rows + b * s_rows);
}
// req[i][j] = T[i][col0 + idx[j]]
__device__ __forceinline__ void gather_columns256_body(u32 nrow, size_t ld, size_t col0, const E* __restrict__ T, const u64* __restrict__ idx, u32 nreq,
                                                       E* __restrict__ req) {
  const u32 t = blockIdx.x * Z_THREADS + threadIdx.x;
  if (t >= nrow * nreq) return;
  const u32 i = t / nreq, j = t % nreq;
  st32(&req[t], ld32(&T[(size_t)i * ld + col0 + idx[j]]));
}
__global__ __launch_bounds__(Z_THREADS) void gather_columns256_kernel(u32 nrow, size_t ld, size_t col0, const E* __restrict__ T, const u64* __restrict__ idx,
                                                                      u32 nreq, E* __restrict__ req) {
  gather_columns256_body(nrow, ld, col0, T, idx, nreq, req);
}
// statement blockIdx.y: idx [nb][nreq], req [nb][nrow][nreq]
__global__ __launch_bounds__(Z_THREADS) void gather_columns256_batch_kernel(u32 nrow, size_t ld, size_t col0, LfBatchPtrs T, const u64* __restrict__ idx, u32 nreq,
                                                                            E* __restrict__ req) {
  const size_t b = blockIdx.y;
  gather_columns256_body(nrow, ld, col0, (const E*)T.p[b], idx + b * nreq, nreq, req + b * (size_t)nrow * nreq);
}

// Quad::bind_gh_all (lib/sumcheck/quad.h:188-210), the verifier's combined bind: the sum over all corners of
// prep_v(v, beta) (EQ(G0,g) + alpha EQ(G1,g)) EQ(H0,h0) EQ(H1,h1); block sums go as limbs into 8 words
__global__ __launch_bounds__(Z_THREADS) void bind_gh_all256_kernel(size_t n, const corner4* __restrict__ t, const E* __restrict__ kvec, const E* __restrict__ eqg,
                                                                   const E* __restrict__ eqh0, const E* __restrict__ eqh1, E beta, u64* __restrict__ acc) {
  __shared__ E sh[Z_THREADS];
  E s = e32_zero();
  for (size_t i = (size_t)blockIdx.x * Z_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * Z_THREADS) {
    const corner4 cr = t[i];
    E v = ld32(&kvec[cr.vi]);
    if (e32_is_zero(v)) v = beta;  // prep_v: assert-zero terms carry beta (quad.h:213-220)
    E qv = fp256_mul(v, ld32(&eqg[cr.g]));
    qv = fp256_mul(qv, ld32(&eqh0[cr.h0]));
    s = fp256_add(s, fp256_mul(qv, ld32(&eqh1[cr.h1])));
  }
  s = block_sum256(s, sh);
  if (threadIdx.x == 0) limbs_atomic_add(acc, s);
}

inline u32 nblk(size_t n, u32 per = Z_THREADS) { return (u32)((n + per - 1) / per ? (n + per - 1) / per : 1); }
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ------------------------------------------------------------------ device steps
int raw_eq2_256(lfgpu_ctx* c, const F256& F, size_t logn, size_t n, const E* G0, const E* G1, const E& alpha, E* d_eq) {
  if (n == 0) return LFGPU_OK;
  std::vector<E> Gt(4 * logn + 1);
  for (size_t l = 0; l < logn; ++l) {
    Gt[l] = G0[l];
    Gt[logn + l] = G1[l];
    Gt[2 * logn + l] = F.sub(F.one, G0[l]);
    Gt[3 * logn + l] = F.sub(F.one, G1[l]);
  }
  const u32 lb = (u32)(logn / 2), hb = (u32)logn - lb;
  const size_t ntab = 2 * (((size_t)1 << lb) + ((size_t)1 << hb));
  void* d_G = nullptr;
  LF_TRY(lf_scratch2(c, (Gt.size() + ntab) * 32 + 64, &d_G));
  E* d_tab = (E*)d_G + Gt.size();
  if (Gt.size() * 32 <= LF_STAGE_SLOT) {  // 4 logn + 1 <= 128 elements: through the pinned ring, no synchronisation
    LF_TRY(lf_stage_upload(c, d_G, Gt.data(), Gt.size() * 32));
  } else {
    LF_HIP(c, hipMemcpyAsync(d_G, Gt.data(), Gt.size() * 32, hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));  // Gt is a local
  }
  if (logn < 6) {  // tiny: the direct product per entry
    hipLaunchKernelGGL(raw_eq2_256_kernel, dim3(nblk(n)), dim3(Z_THREADS), 0, c->stream, (u32)logn, (u32)n, (const E*)d_G, alpha, F.one, d_eq);
  } else {
    hipLaunchKernelGGL(eq_tables256_kernel, dim3(nblk(ntab)), dim3(Z_THREADS), 0, c->stream, (u32)logn, lb, (const E*)d_G, alpha, F.one, d_tab);
    hipLaunchKernelGGL(raw_eq2_split256_kernel, dim3(nblk(n)), dim3(Z_THREADS), 0, c->stream, (u32)logn, lb, (u32)n, (const E*)d_tab, d_eq);
  }
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}

typedef void (*round256_fn)(void* user, size_t hand, size_t rnd, const E ev[3], E* chal);

// The merge structure of HQuad::bind_h at round-hand rh (per-block output offsets + the size after the bind) is a circuit
// constant: counted from the corners `hc` (nh entries) by the first call that reaches the round-hand on a per-launch path, kept
// with the quad from then on.  The single and the batched layer both record through here, so either may run first on a quad.
int bind_shape256(lfgpu_quad* q, size_t rh, size_t nh, const uint2* hc, int hand) {
  lfgpu_ctx* c = q->c;
  if (q->bind_shape.size() <= rh) q->bind_shape.resize(rh + 1, lfgpu_quad::BindShape{nullptr, 0, 0});
  lfgpu_quad::BindShape& bs = q->bind_shape[rh];
  if (!nh || (bs.d_off && bs.n_in == nh)) return LFGPU_OK;
  const u32 nbh = nblk(nh);
  if (bs.d_off) (void)hipFree(bs.d_off);
  bs = lfgpu_quad::BindShape{nullptr, nh, 0};
  if (hipMalloc((void**)&bs.d_off, (size_t)nbh * 4) != hipSuccess) return lf_fail(c, LFGPU_ERR_NOMEM, "sumcheck_layer256: bind offsets");
  u32* total = (u32*)((uint8_t*)c->mailbox_d + 64);
  hipLaunchKernelGGL(hquad_count256_kernel, dim3(nbh), dim3(Z_THREADS), 0, c->stream, nh, hc, hand, bs.d_off);
  hipLaunchKernelGGL(scan256_kernel, dim3(1), dim3(1024), 0, c->stream, nbh, bs.d_off, total);
  u32 tot = 0;
  LF_HIP(c, hipMemcpyAsync(&tot, total, 4, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipStreamSynchronize(c->stream));
  bs.n_out = tot;
  return LFGPU_OK;
}

// One layer of the sumcheck (ProverLayers::layer): bind_g, then per round and hand the QW scatter, the two partial sums
// (one read-back), the caller's transcript step, Dense::bind and HQuad::bind_h.  d_W (the layer's inputs) is left intact:
// both hands bind into ping-pong buffers.
int sumcheck_layer256(lfgpu_quad* q, const F256& F, size_t logv, const E* G0, const E* G1, const E& alpha, const E& beta, size_t logw, size_t nw,
                      const E* d_W, const E wc_in[2], round256_fn round, void* user, E wc_out[2], E* g_out /*[2][logw]*/, E* bound_quad) {
  lfgpu_ctx* c = q->c;
  if (nw == 0 || logw > 40 || nw > ((size_t)1 << logw) || nw <= q->hmax) return lf_fail(c, LFGPU_ERR_ARG, "sumcheck_layer256: nw must exceed the largest hand index");
  if (logv > 40 || ((size_t)1 << logv) < q->nv) return lf_fail(c, LFGPU_ERR_ARG, "sumcheck_layer256: 2^logv < nv");
  const size_t nt = q->n, nh0 = q->nh0, half = (nw + 1) / 2;
  // scratch: eq | limb accumulators (bind_g runs, then the QW of every round-hand; self-cleaning) | hc[2] | vc[2] |
  // 4 half hand buffers | the round's two sums as limbs
  const size_t acc_n = std::max(nh0, nw);
  const size_t grid_bytes = acc_n * 64 + sizeof(Grid256Sync) + G256_WGS * 4 + nh0 * 4 + 256;  // second accumulator array, barrier state, counts, src
  const size_t bytes = q->nv * 32 + acc_n * 64 + 2 * nh0 * 8 + 2 * nh0 * 32 + 4 * half * 32 + 256 + 1024 + grid_bytes;
  void* sc = nullptr;
  LF_TRY(lf_scratch(c, bytes, &sc));
  uint8_t* b = (uint8_t*)sc;
  E* d_eq = (E*)b;                     b += q->nv * 32;
  u64* acc = (u64*)b;                  b += acc_n * 64;
  uint2* hc[2] = {(uint2*)b, (uint2*)(b + nh0 * 8)};  b += 2 * nh0 * 8;
  b = (uint8_t*)(((uintptr_t)b + 31) & ~(uintptr_t)31);
  E* vc[2] = {(E*)b, (E*)b + nh0};     b += 2 * nh0 * 32;
  E* wb[2][2] = {{(E*)b, (E*)b + half}, {(E*)b + 2 * half, (E*)b + 3 * half}};  b += 4 * half * 32;
  u64* d_sums = (u64*)b;
  u32* d_done = (u32*)(d_sums + 16);
  b += 256;
  u64* acc2 = (u64*)b;                 b += acc_n * 64;
  Grid256Sync* gsync = (Grid256Sync*)b; b += sizeof(Grid256Sync);
  u32* g_counts = (u32*)b;             b += G256_WGS * 4;
  u32* g_src = (u32*)b;
  volatile u64* post = c->poll_h + 256;  // coherent pinned words a running kernel writes and the host polls (ctx.h)
  volatile u64* cmd = c->poll_h + 320;   // ... and the host's answers (the challenge as tagged words)
  // Quad::bind_g
  LF_TRY(raw_eq2_256(c, F, logv, q->nv, G0, G1, alpha, d_eq));
  LF_HIP(c, hipMemsetAsync(acc, 0, acc_n * 64, c->stream));
  LF_HIP(c, hipMemsetAsync(d_sums, 0, 192, c->stream));  // the 16 sum words + the block counter
  hipLaunchKernelGGL(bindg_emit256_kernel, dim3(nblk(nt, BG_THREADS)), dim3(BG_THREADS), 0, c->stream, nt, (const corner4*)q->d_morton, (const E*)q->d_kvec,
                     (const E*)d_eq, beta, (const u32*)q->d_runoff, hc[0], acc);
  hipLaunchKernelGGL(limb_normalize256_kernel, dim3(nblk(nh0)), dim3(Z_THREADS), 0, c->stream, nh0, acc, F.rsq, vc[0]);
  LF_HIP(c, hipGetLastError());
  size_t nh = nh0;
  int cur = 0;
  E sum = F.add(wc_in[0], F.mul(alpha, wc_in[1]));
  const E* WH[2] = {d_W, d_W};
  size_t nW[2] = {nw, nw};
  int wsel[2] = {0, 0};
  if (q->bind_shape.size() < 2 * logw) q->bind_shape.resize(2 * logw, lfgpu_quad::BindShape{nullptr, 0, 0});
  u64 h_sums[16];
  E* h_out = (E*)c->mailbox_h;
  auto wait_post = [&](u64 seq) -> int {  // bounded: a kernel that is over without posting is an error
    // The stream is only looked at after 50 ms without the post (a dead kernel must not hang the caller): in a healthy run no HIP
    // call is made while a resident kernel waits for this thread.  It matters -- another thread's hipFree holds the runtime's
    // lock while it waits for every stream of the device, hence for that kernel; a hipStreamQuery here would wait for the lock
    // and the kernel for its challenge until its timeout.
    u64 spins = 0;
    double t_first = 0;
    while (__atomic_load_n((const u64*)&post[16], __ATOMIC_ACQUIRE) != seq) {
      if (spins > 0x8000 && (spins & 0xff) == 0) sched_yield();  // see sc_wait_post (sumcheck.hip)
      if ((++spins & 0xfff) == 0) {
        const double t = now_ms();
        if (t_first == 0) t_first = t;
        if (t - t_first < 50.0) continue;
        const hipError_t qe = hipStreamQuery(c->stream);
        if (qe == hipSuccess) {
          if (__atomic_load_n((const u64*)&post[16], __ATOMIC_ACQUIRE) == seq) break;
          return lf_fail(c, LFGPU_ERR_ASSERT, "sumcheck_layer256: kernel finished without posting");
        }
        if (qe != hipErrorNotReady) return lf_fail(c, LFGPU_ERR_HIP, "sumcheck_layer256: %s", hipGetErrorString(qe));
      }
    }
    return LFGPU_OK;
  };
  // LFGPU_P256_GRID [1]: once the HQUAD and both hand arrays have <= G256_MAX entries the rest of the layer is ONE launch of
  // co-resident workgroups that take every challenge through pinned memory (grid256_layer_kernel); 0 = three launches per
  // round-hand throughout (A/B, and the fallback where a running kernel cannot see host writes)
  static const int grid_env = getenv("LFGPU_P256_GRID") ? atoi(getenv("LFGPU_P256_GRID")) : 1;
  bool grid_ok = grid_env && lf_sc_resident_ok(c) && c->grid_strikes < 2;
  struct CuGuard {  // the grid's CUs go back to the device's budget (ctx.h) however this function is left, after the kernel has ended
    lfgpu_ctx* c;
    ~CuGuard() {
      if (c->cu_held) {
        (void)hipStreamSynchronize(c->stream);
        lf_cu_release(c, -1);
      }
    }
  } cu_guard{c};
  for (size_t rnd = 0; rnd < logw; ++rnd)
    for (int hand = 0; hand < 2; ++hand) {
      // hand-off point: above it a round-hand is three launches spread over the whole chip.  Measured on the mdoc signature
      // circuit (sumcheck ms): no grid 19.8; grid from 1024 / 2048 / 8192 / 32768 / 131072 entries on: 19.1 / 19.1 / 19.8 / 20.0 /
      // 20.1.  With LFGPU_VERBOSE the host's turn shows as 1.2 us per round-hand and the wait for the device as 23 us for a
      // layer that starts at 409 entries (one workgroup) up to 41 us from 69150: ~5000 instructions on the critical path of a
      // round-hand (0.82 us per product, tools/ubench_p256; the 8-wave sum with its serial tail; the recomputed bound hand
      // entry) at the one-instruction-per-5.6-cycles issue rate of a lone wave -- not launches, barriers or memory round trips
      // (an LDS-resident tail for <= 512 entries was built and measured: no change)
      static const size_t grid_max = [] {
        const char* e = getenv("LFGPU_P256_GRID_MAX");
        return std::min<size_t>(e ? (size_t)atol(e) : (size_t)2048, G256_MAX);
      }();
      static const u32 grid_per_wg = getenv("LFGPU_P256_PER_WG") ? (u32)std::max(64, atoi(getenv("LFGPU_P256_PER_WG"))) : 512u;
      u32 want_G = 0;  // workgroups of the grid this round-hand could hand the layer to (0: not now)
      if (grid_ok && nh <= grid_max && nW[0] <= grid_max && nW[1] <= grid_max) {
        int pc = 0;  // all of them must be resident together (they synchronise through device memory): one fits a CU ...
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, (const void*)grid256_layer_kernel, G256_THREADS, 0) != hipSuccess) pc = 0;
        if (pc < 1) return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "sumcheck_layer256: the grid kernel does not fit a CU");
        const size_t big = std::max(nh, std::max(nW[0], nW[1]));
        want_G = std::min<u32>(std::max<u32>((u32)((big + grid_per_wg - 1) / grid_per_wg), 1), std::min<u32>(G256_WGS, (u32)c->num_cu));
      }
      // ... and the device's CU budget must have room for them (ctx.h); without it this round-hand takes the three launches
      // below and the next one asks again
      if (want_G && lf_cu_acquire(c, (int)want_G)) {
        const u32 per_wg = grid_per_wg, G = want_G;
        const size_t big = std::max(nh, std::max(nW[0], nW[1]));
        Grid256 a{};
        a.hcA = hc[cur];
        a.vcA = vc[cur];
        a.hcB = hc[1 - cur];
        a.vcB = vc[1 - cur];
        a.nh = (u32)nh;
        for (int h = 0; h < 2; ++h) {
          a.W[h] = WH[h];
          a.nW[h] = (u32)nW[h];
          a.Wb[h][0] = wb[h][0];
          a.Wb[h][1] = wb[h][1];
        }
        a.QW = acc;
        a.QW2 = acc2;
        a.rh0 = (u32)(2 * rnd + hand);
        a.rh1 = (u32)(2 * logw);
        a.seq0 = c->poll_seq + 1;
        c->poll_seq += (a.rh1 - a.rh0) + 1;
        a.timeout_ticks = 5000ull * c->wall_khz;
        a.post = post;
        a.cmd = cmd;
        a.gs = gsync;
        a.counts = g_counts;
        a.src = g_src;
        a.per_wg = per_wg;
        static const int wave_tail_env = getenv("LFGPU_P256_WAVE_TAIL") ? atoi(getenv("LFGPU_P256_WAVE_TAIL")) : 1;
        a.wave_tail = (u32)wave_tail_env;
        a.rsq = F.rsq;
        static const u64 place_ms = getenv("LFGPU_SC_PLACE_MS") ? (u64)std::max(1, atoi(getenv("LFGPU_SC_PLACE_MS"))) : 250ull;
        a.place_ticks = place_ms * c->wall_khz;
        {  // test hook: the first LFGPU_P256_TEST_DROP grid launches of the process lose their last workgroup
          static std::atomic<int> drops{getenv("LFGPU_P256_TEST_DROP") ? atoi(getenv("LFGPU_P256_TEST_DROP")) : 0};
          if (G > 1 && drops.load() > 0 && drops.fetch_sub(1) > 0) a.test_drop = 1;
        }
        LF_HIP(c, hipMemsetAsync(gsync, 0, sizeof(Grid256Sync), c->stream));
        hipLaunchKernelGGL(grid256_layer_kernel, dim3(G), dim3(G256_THREADS), 0, c->stream, a);
        LF_HIP(c, hipGetLastError());
        u64 seq = a.seq0;
        size_t r2 = rnd;
        bool not_placed = false;
        static const bool verbose = getenv("LFGPU_VERBOSE") != nullptr;
        double t_wait = 0, t_host = 0, tp0 = verbose ? now_ms() : 0;
        for (u32 rh = a.rh0; rh < a.rh1; ++rh, ++seq) {
          const int hd = (int)(rh & 1);
          r2 = rh >> 1;
          LF_TRY(wait_post(seq));
          if (verbose) {
            const double t = now_ms();
            t_wait += t - tp0;
            tp0 = t;
          }
          if (post[9] == 2 && rh == a.rh0) {  // the grid was not placed whole: nothing but scratch was written
            not_placed = true;
            break;
          }
          if (post[9] != 0)
            return lf_fail(c, LFGPU_ERR_ASSERT, "sumcheck_layer256: the grid kernel timed out waiting for a challenge (status %llu at round-hand %u of [%u, %u), %u workgroups)",
                           (unsigned long long)post[9], rh, a.rh0, a.rh1, G);
          E coef[3], ev[3], r;
          for (int k = 0; k < 4; ++k) {
            coef[0].l[k] = post[k];
            coef[2].l[k] = post[4 + k];
          }
          coef[1] = F.sub(F.sub(F.sub(sum, coef[0]), coef[0]), coef[2]);
          for (int k = 0; k < 3; ++k) ev[k] = F.eval_monomial(coef, F.pts[k]);
          round(user, (size_t)hd, r2, ev, &r);
          g_out[hd * logw + r2] = r;
          sum = F.eval_lagrange(ev, r);
          const u64 tag = (seq & 0xffffffffull) << 32;  // eight tagged words: valid as soon as all eight carry the tag
          for (int k = 0; k < 8; ++k) __atomic_store_n((u64*)&cmd[k], tag | ((r.l[k >> 1] >> (32 * (k & 1))) & 0xffffffffull), __ATOMIC_RELAXED);
          __atomic_thread_fence(__ATOMIC_RELEASE);
          if (verbose) {
            const double t = now_ms();
            t_host += t - tp0;
            tp0 = t;
          }
        }
        if (verbose)
          fprintf(stderr, "lfgpu sumcheck_layer256 grid: %u round-hands from %zu entries: waiting for the device %.1f us, host's turn %.1f us per round-hand\n",
                  a.rh1 - a.rh0, big, 1e3 * t_wait / (a.rh1 - a.rh0), 1e3 * t_host / (a.rh1 - a.rh0));
        if (not_placed) {  // another process holds CUs (the budget rules it out within this one): per-launch kernels from here on
          LF_HIP(c, hipStreamSynchronize(c->stream));
          lf_cu_release(c, -1);
          grid_ok = false;
          ++c->grid_strikes;
          LF_HIP(c, hipMemsetAsync(acc, 0, acc_n * 64, c->stream));  // the kernel's clears / first sums may have touched the accumulators
          if (verbose) fprintf(stderr, "lfgpu sumcheck_layer256: resident grid not placed (strike %d): per-launch kernels for this layer\n", c->grid_strikes);
        } else {
        LF_TRY(wait_post(seq));  // the layer's last post: W[0][0], W[1][0], the HQUAD scalar
        lf_cu_release(c, -1);
        if (post[9] != 0 || post[8] != 1) return lf_fail(c, LFGPU_ERR_ASSERT, "sumcheck_layer256: HQUAD did not fold to one entry (%llu)", (unsigned long long)post[8]);
        for (int k = 0; k < 4; ++k) {
          wc_out[0].l[k] = post[k];
          wc_out[1].l[k] = post[4 + k];
          if (bound_quad) bound_quad->l[k] = post[12 + k];
        }
        return LFGPU_OK;
        }
      }
      // QW scatter (prover_layers.h:239-243) + evaluations: two launches, one read-back
      if (nh) hipLaunchKernelGGL(qw_scatter256_kernel, dim3(nblk(nh)), dim3(Z_THREADS), 0, c->stream, nh, (const uint2*)hc[cur], (const E*)vc[cur], hand,
                                 WH[1 - hand], acc);
      const u64 seq = ++c->poll_seq;
      hipLaunchKernelGGL(partials256_kernel, dim3(std::min<u32>(nblk(nW[hand] / 2), 256)), dim3(Z_THREADS), 0, c->stream, nW[hand], acc, F.rsq, WH[hand], d_sums,
                         d_done, post, seq);
      LF_HIP(c, hipGetLastError());
      LF_TRY(wait_post(seq));
      for (int k = 0; k < 16; ++k) h_sums[k] = post[k];
      // coef[0] = a0, coef[2] = a2, coef[1] from the running sum (prover_layers.h:390-396, logc = 0)
      E coef[3], ev[3], r;
      coef[0] = fp256_reduce_limbs(h_sums, F.rsq);
      coef[2] = fp256_reduce_limbs(h_sums + 8, F.rsq);
      coef[1] = F.sub(F.sub(F.sub(sum, coef[0]), coef[0]), coef[2]);
      for (int k = 0; k < 3; ++k) ev[k] = F.eval_monomial(coef, F.pts[k]);
      round(user, (size_t)hand, rnd, ev, &r);
      g_out[hand * logw + rnd] = r;
      sum = F.eval_lagrange(ev, r);
      // Dense::bind of this hand + HQuad::bind_h: one launch.  The merge structure of a round-hand is a circuit constant:
      // counted at the first proof, kept with the layer from then on
      const u32 nbh = nh ? nblk(nh) : 0, nbd = nblk((nW[hand] + 1) / 2);
      LF_TRY(bind_shape256(q, 2 * rnd + hand, nh, hc[cur], hand));
      lfgpu_quad::BindShape& bs = q->bind_shape[2 * rnd + hand];
      E* dst = wb[hand][wsel[hand]];
      hipLaunchKernelGGL(bind256_kernel, dim3(nbd + nbh), dim3(Z_THREADS), 0, c->stream, nbd, nW[hand], WH[hand], dst, nh, (const uint2*)hc[cur],
                         (const E*)vc[cur], r, hand, (const u32*)bs.d_off, hc[1 - cur], vc[1 - cur]);
      LF_HIP(c, hipGetLastError());
      WH[hand] = dst;
      wsel[hand] ^= 1;
      nW[hand] = (nW[hand] + 1) / 2;
      if (nh) {
        nh = bs.n_out;
        cur = 1 - cur;
      }
    }
  // W[0][0], W[1][0] and the bound quad (the HQUAD has shrunk to one entry)
  if (nh != 1) return lf_fail(c, LFGPU_ERR_ASSERT, "sumcheck_layer256: HQUAD did not fold to one entry (%zu)", nh);
  LF_HIP(c, hipMemcpyAsync(&h_out[0], WH[0], 32, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipMemcpyAsync(&h_out[1], WH[1], 32, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipMemcpyAsync(&h_out[2], vc[cur], 32, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipStreamSynchronize(c->stream));
  wc_out[0] = h_out[0];
  wc_out[1] = h_out[1];
  if (bound_quad) *bound_quad = h_out[2];
  return LFGPU_OK;
}

// ------------------------------------------------------------------ the batch axis (K14 over Fp256Base)
typedef void (*round_batch256_fn)(void* user, size_t hand, size_t rnd, size_t nb, const uint64_t (*ev)[3][4], uint64_t (*chal)[4]);

int scb256_mailbox(lfgpu_ctx* c) {
  if (c->sc_batch256_h) return LFGPU_OK;
  void* p = nullptr;
  const size_t bytes = (size_t)LFGPU_SC_BATCH_MAX * SCB256_SLOT_WORDS * 8;
  if (hipHostMalloc(&p, bytes, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
    (void)hipGetLastError();
    return lf_fail(c, LFGPU_ERR_NOMEM, "sumcheck_layer_batch256: the pinned mailbox");
  }
  memset(p, 0, bytes);
  c->sc_batch256_h = (volatile u64*)p;
  return LFGPU_OK;
}
// one spin for all B slots (lf_scb_wait, sumcheck.hip: the stream is looked at after 50 ms without a post)
int scb256_wait(lfgpu_ctx* c, size_t B, u64 seq) {
  volatile u64* const mb = c->sc_batch256_h;
  u64 spins = 0;
  double t_first = 0;
  for (size_t b = 0; b < B;) {
    const u64* w = (const u64*)&mb[b * SCB256_SLOT_WORDS + 16];
    if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == seq) {
      ++b;
      continue;
    }
    if (spins > 0x8000 && (spins & 0xff) == 0) sched_yield();
    if ((++spins & 0xfff) == 0) {
      const double t = now_ms();
      if (t_first == 0) t_first = t;
      if (t - t_first < 50.0) continue;
      const hipError_t qe = hipStreamQuery(c->stream);
      if (qe == hipSuccess) {  // the kernel is over: every post must be visible now
        if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == seq) continue;
        return lf_fail(c, LFGPU_ERR_ASSERT, "sumcheck_layer_batch256: kernel finished without posting statement %zu", b);
      }
      if (qe != hipErrorNotReady) return lf_fail(c, LFGPU_ERR_HIP, "sumcheck_layer_batch256: %s", hipGetErrorString(qe));
    }
  }
  return LFGPU_OK;
}

// Eqs::raw_eq2 of B point sets in one upload and one launch chain.  The uploaded table holds, per statement, the 4 logn
// elements of raw_eq2_256 followed by alpha and beta (gs = 4 logn + 2 elements); it stays in scratch2 for the batched bind_g,
// which reads beta from it.  *d_pts_out: the device table.
int raw_eq2_256_batch(lfgpu_ctx* c, const F256& F, size_t B, size_t logn, size_t n, const E* G0, const E* G1, const E* alpha, const E* beta, E* d_eq,
                      const E** d_pts_out) {
  const size_t gs = 4 * logn + 2;
  std::vector<E> Gt(B * gs);
  for (size_t b = 0; b < B; ++b) {
    E* g = &Gt[b * gs];
    for (size_t l = 0; l < logn; ++l) {
      g[l] = G0[b * logn + l];
      g[logn + l] = G1[b * logn + l];
      g[2 * logn + l] = F.sub(F.one, G0[b * logn + l]);
      g[3 * logn + l] = F.sub(F.one, G1[b * logn + l]);
    }
    g[4 * logn] = alpha[b];
    g[4 * logn + 1] = beta[b];
  }
  const u32 lb = (u32)(logn / 2), hb = (u32)logn - lb;
  const size_t ntab = 2 * (((size_t)1 << lb) + ((size_t)1 << hb));
  void* d_G = nullptr;
  LF_TRY(lf_scratch2(c, B * (gs + ntab) * 32 + 64, &d_G));
  E* d_tab = (E*)d_G + B * gs;
  LF_HIP(c, hipMemcpyAsync(d_G, Gt.data(), Gt.size() * 32, hipMemcpyHostToDevice, c->stream));
  LF_HIP(c, hipStreamSynchronize(c->stream));  // Gt is a local
  *d_pts_out = (const E*)d_G;
  if (n == 0) return LFGPU_OK;
  if (logn < 6) {
    hipLaunchKernelGGL(raw_eq2_256_batch_kernel, dim3(nblk(n), (u32)B), dim3(Z_THREADS), 0, c->stream, (u32)logn, (u32)n, (const E*)d_G, gs, F.one, d_eq);
  } else {
    hipLaunchKernelGGL(eq_tables256_batch_kernel, dim3(nblk(ntab), (u32)B), dim3(Z_THREADS), 0, c->stream, (u32)logn, lb, (const E*)d_G, gs, F.one, d_tab, ntab);
    hipLaunchKernelGGL(raw_eq2_split256_batch_kernel, dim3(nblk(n), (u32)B), dim3(Z_THREADS), 0, c->stream, (u32)logn, lb, (u32)n, (const E*)d_tab, ntab, d_eq);
  }
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}

// sumcheck_layer256 for B statements of one quad in lock-step.  Only the values (vc), the hand arrays, the accumulators and the
// sums carry a statement stride; the corners, the merge structure and the recorded bind shapes are the circuit's.  No resident
// grid: above SCB256_SMALL_MAX a round-hand is three launches of B times the single call's blocks, at or below it one launch
// of B workgroups (LFGPU_P256_BATCH_SMALL = 0: three launches throughout).  d_W is left intact.
int sumcheck_layer_batch256(lfgpu_quad* q, const F256& F, size_t B, size_t logv, const E* G0, const E* G1, const E* alpha, const E* beta, size_t logw, size_t nw,
                            const E* d_W, size_t ldw, const E* wc_in /*[B][2]*/, round_batch256_fn round, void* user, E* wc_out /*[B][2]*/,
                            E* g_out /*[B][2][logw]*/, E* bound_quad /*[B] or nullptr*/) {
  lfgpu_ctx* c = q->c;
  const size_t nt = q->n, nh0 = q->nh0, half = (nw + 1) / 2, nv = q->nv;
  const size_t acc_n = std::max(nh0, nw);
  // scratch per statement: eq | limb accumulators (64 bytes per entry) | 2 HQUAD value arrays | 4 half hand buffers | sums;
  // shared: the two corner arrays
  const size_t per = nv * 32 + acc_n * 64 + 2 * nh0 * 32 + 4 * half * 32 + 16 * 8 + 64 + 3 * 32;
  if ((acc_n >> 32) || per > ((size_t)1 << 40) / B) return lf_fail(c, LFGPU_ERR_NOMEM, "sumcheck_layer_batch256: %zu bytes of scratch per statement, %zu statements", per, B);
  void* sc = nullptr;
  LF_TRY(lf_scratch(c, B * per + 2 * nh0 * 8 + 1024, &sc));
  LF_TRY(scb256_mailbox(c));
  volatile u64* const mb = c->sc_batch256_h;
  uint8_t* p = (uint8_t*)sc;
  E* d_eq = (E*)p;                      p += B * nv * 32;
  u64* acc = (u64*)p;                   p += B * acc_n * 64;
  E* vc[2] = {(E*)p, (E*)p + B * nh0};  p += 2 * B * nh0 * 32;
  E* wb[2][2];
  for (int k = 0; k < 4; ++k) {
    wb[k >> 1][k & 1] = (E*)p;
    p += B * half * 32;
  }
  E* d_out = (E*)p;                     p += B * 3 * 32;
  u64* d_sums = (u64*)p;                p += B * 16 * 8;
  u32* d_done = (u32*)p;                p += B * 64;
  uint2* hc[2] = {(uint2*)p, (uint2*)p + nh0};
  const size_t s_acc = acc_n * 8;  // words between two statements' accumulators
  // Quad::bind_g of all statements: the EQ vectors, the runs, their normalisation
  const E* d_pts = nullptr;
  LF_TRY(raw_eq2_256_batch(c, F, B, logv, nv, G0, G1, alpha, beta, d_eq, &d_pts));
  LF_HIP(c, hipMemsetAsync(acc, 0, B * acc_n * 64, c->stream));
  LF_HIP(c, hipMemsetAsync(d_sums, 0, B * (16 * 8 + 64), c->stream));  // the sum words + the block counters
  hipLaunchKernelGGL(bindg_emit256_batch_kernel, dim3(nblk(nt, BG_THREADS), (u32)B), dim3(BG_THREADS), 0, c->stream, nt, (const corner4*)q->d_morton,
                     (const E*)q->d_kvec, (const E*)d_eq, nv, d_pts, 4 * logv + 2, (u32)(4 * logv + 1), (const u32*)q->d_runoff, hc[0], acc, s_acc);
  hipLaunchKernelGGL(limb_normalize256_batch_kernel, dim3(nblk(nh0), (u32)B), dim3(Z_THREADS), 0, c->stream, nh0, acc, s_acc, F.rsq, vc[0], nh0);
  LF_HIP(c, hipGetLastError());
  size_t nh = nh0;
  int cur = 0;
  std::vector<E> sum(B);
  for (size_t b = 0; b < B; ++b) sum[b] = F.add(wc_in[2 * b], F.mul(alpha[b], wc_in[2 * b + 1]));
  const E* WH[2] = {d_W, d_W};
  size_t sW[2] = {ldw, ldw};
  size_t nW[2] = {nw, nw};
  int wsel[2] = {0, 0};
  // LFGPU_P256_BATCH_SMALL [1]: 0 = three launches per round-hand throughout (A/B: the same bytes)
  static const int small_env = getenv("LFGPU_P256_BATCH_SMALL") ? atoi(getenv("LFGPU_P256_BATCH_SMALL")) : 1;
  if (small_env && !(c->attr_done & 32u)) {
    LF_HIP(c, hipFuncSetAttribute((const void*)sc_small_step_batch256_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SCB256_SMALL_LDS));
    c->attr_done |= 32u;
  }
  Chal256 ch{};
  bool pending = false;  // the binds of round-hand prh with the challenges in ch ride at the head of the next fused step
  size_t prh = 0;
  // the fused step: [pending binds] + [scatter, sums and post of eval_hand]
  auto small_step = [&](int do_eval, int eval_hand, u64 seq) -> int {
    Small256 a{};
    a.do_bind = pending ? 1 : 0;
    a.do_eval = do_eval;
    a.eval_hand = eval_hand;
    a.hc_in = hc[cur];
    a.vc_in = vc[cur];
    a.s_vc = nh0;
    a.nh = (u32)nh;
    for (int k = 0; k < 2; ++k) {
      a.W[k] = WH[k];
      a.s_W[k] = sW[k];
      a.nW[k] = (u32)nW[k];
    }
    a.rsq = F.rsq;
    int ph = 0;
    if (pending) {
      ph = (int)(prh & 1);
      LF_TRY(bind_shape256(q, prh, nh, hc[cur], ph));
      const lfgpu_quad::BindShape& bs = q->bind_shape[prh];
      a.bind_hand = ph;
      a.hc_out = hc[1 - cur];
      a.vc_out = vc[1 - cur];
      a.nh_out = (u32)bs.n_out;
      a.block_off = bs.d_off;
      a.Wdst = wb[ph][wsel[ph]];
      a.s_Wdst = half;
    }
    hipLaunchKernelGGL(sc_small_step_batch256_kernel, dim3((u32)B), dim3(Z_THREADS), SCB256_SMALL_LDS, c->stream, a, ch, mb, seq);
    LF_HIP(c, hipGetLastError());
    if (pending) {
      WH[ph] = a.Wdst;
      sW[ph] = half;
      wsel[ph] ^= 1;
      nW[ph] = (nW[ph] + 1) / 2;
      if (nh) {
        nh = a.nh_out;
        cur = 1 - cur;
      }
      pending = false;
    }
    return LFGPU_OK;
  };
  std::vector<uint64_t> evw(B * 12), rr(B * 4);
  std::vector<E> ev(3 * B);
  for (size_t rnd = 0; rnd < logw; ++rnd)
    for (int hand = 0; hand < 2; ++hand) {
      const bool fused = small_env && std::max(nh, std::max(nW[0], nW[1])) <= SCB256_SMALL_MAX;
      const u64 seq = ++c->poll_seq;
      if (fused) {
        LF_TRY(small_step(1, hand, seq));
      } else {
        if (nh) hipLaunchKernelGGL(qw_scatter256_batch_kernel, dim3(nblk(nh), (u32)B), dim3(Z_THREADS), 0, c->stream, nh, (const uint2*)hc[cur], (const E*)vc[cur], nh0,
                                   hand, WH[1 - hand], sW[1 - hand], acc, s_acc);
        hipLaunchKernelGGL(partials256_batch_kernel, dim3(std::min<u32>(nblk(nW[hand] / 2), 256), (u32)B), dim3(Z_THREADS), 0, c->stream, nW[hand], acc, s_acc, F.rsq,
                           WH[hand], sW[hand], d_sums, d_done, mb, seq);
        LF_HIP(c, hipGetLastError());
      }
      LF_TRY(scb256_wait(c, B, seq));
      // per statement as in sumcheck_layer256: coef[0] = a0, coef[2] = a2, coef[1] from the running sum
      for (size_t b = 0; b < B; ++b) {
        u64 w[16];
        for (int k = 0; k < 16; ++k) w[k] = mb[b * SCB256_SLOT_WORDS + k];
        E coef[3];
        coef[0] = fp256_reduce_limbs(w, F.rsq);
        coef[2] = fp256_reduce_limbs(w + 8, F.rsq);
        coef[1] = F.sub(F.sub(F.sub(sum[b], coef[0]), coef[0]), coef[2]);
        for (int k = 0; k < 3; ++k) {
          ev[3 * b + k] = F.eval_monomial(coef, F.pts[k]);
          memcpy(&evw[12 * b + 4 * k], ev[3 * b + k].l, 32);
        }
      }
      round(user, (size_t)hand, rnd, B, (const uint64_t(*)[3][4])evw.data(), (uint64_t(*)[4])rr.data());
      for (size_t b = 0; b < B; ++b) {
        E r;
        memcpy(r.l, &rr[4 * b], 32);
        g_out[(b * 2 + hand) * logw + rnd] = r;
        sum[b] = F.eval_lagrange(&ev[3 * b], r);
        ch.r[b] = r;
      }
      if (fused) {
        pending = true;
        prh = 2 * rnd + hand;
        continue;
      }
      // Dense::bind of this hand + HQuad::bind_h of all statements: one launch
      const u32 nbh = nh ? nblk(nh) : 0, nbd = nblk((nW[hand] + 1) / 2);
      LF_TRY(bind_shape256(q, 2 * rnd + hand, nh, hc[cur], hand));
      const lfgpu_quad::BindShape& bs = q->bind_shape[2 * rnd + hand];
      E* dst = wb[hand][wsel[hand]];
      hipLaunchKernelGGL(bind256_batch_kernel, dim3(nbd + nbh, (u32)B), dim3(Z_THREADS), 0, c->stream, nbd, nW[hand], WH[hand], sW[hand], dst, half, nh,
                         (const uint2*)hc[cur], (const E*)vc[cur], nh0, ch, hand, (const u32*)bs.d_off, hc[1 - cur], vc[1 - cur]);
      LF_HIP(c, hipGetLastError());
      WH[hand] = dst;
      sW[hand] = half;
      wsel[hand] ^= 1;
      nW[hand] = (nW[hand] + 1) / 2;
      if (nh) {
        nh = bs.n_out;
        cur = 1 - cur;
      }
    }
  if (pending) LF_TRY(small_step(0, 0, 0));  // the last binds
  if (nh != 1) return lf_fail(c, LFGPU_ERR_ASSERT, "sumcheck_layer_batch256: HQUAD did not fold to one entry (%zu)", nh);
  hipLaunchKernelGGL(readout256_batch_kernel, dim3(1), dim3(Z_THREADS), 0, c->stream, (u32)B, WH[0], sW[0], WH[1], sW[1], (const E*)vc[cur], nh0, d_out);
  LF_HIP(c, hipGetLastError());
  std::vector<E> h_out(3 * B);
  LF_HIP(c, hipMemcpyAsync(h_out.data(), d_out, 3 * B * 32, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipStreamSynchronize(c->stream));
  for (size_t b = 0; b < B; ++b) {
    wc_out[2 * b] = h_out[3 * b];
    wc_out[2 * b + 1] = h_out[3 * b + 1];
    if (bound_quad) bound_quad[b] = h_out[3 * b + 2];
  }
  return LFGPU_OK;
}
}  // namespace

// ------------------------------------------------------------------ the sumcheck layer of Fp256Base behind the kernel ABI
static_assert(LFGPU_SC_BATCH_MAX * 3 <= Z_THREADS, "readout256_batch_kernel: one block reads all statements out");
static inline E e_of(const uint64_t* w) {
  E e;
  memcpy(e.l, w, 32);
  return e;
}
static inline std::vector<E> es_of(const void* w, size_t n) {
  std::vector<E> v(n + 1);
  if (n) memcpy((void*)v.data(), w, n * 32);
  return v;
}
namespace {
struct Tramp256 {
  lfgpu_sc_round256_fn fn;
  void* user;
};
void tramp256_cb(void* u, size_t hand, size_t rnd, const E ev[3], E* chal) {
  const Tramp256* t = (const Tramp256*)u;
  uint64_t e[3][4], r[4];
  for (int k = 0; k < 3; ++k) memcpy(e[k], ev[k].l, 32);
  t->fn(t->user, hand, rnd, e, r);
  memcpy(chal->l, r, 32);
}
}  // namespace

extern "C" int lfgpu_sumcheck_layer256(lfgpu_quad* q, size_t logv, const void* h_G0, const void* h_G1, const uint64_t alpha[4], const uint64_t beta[4],
                                       size_t logw, size_t nw, const void* d_W, const uint64_t wc_in[2][4], lfgpu_sc_round256_fn round, void* user,
                                       uint64_t wc_out[2][4], uint64_t* g_out, uint64_t bound_quad[4]) {
  if (!q) return LFGPU_ERR_ARG;
  lfgpu_ctx* c = q->c;
  if (!alpha || !beta || !d_W || !wc_in || !round || !wc_out || (logw && !g_out) || (logv && (!h_G0 || !h_G1)))
    return lf_fail(c, LFGPU_ERR_ARG, "sumcheck_layer256: null argument");
  if (q->field != LFGPU_FIELD_P256) return lf_fail(c, LFGPU_ERR_ARG, "sumcheck_layer256: the quad is over a 16-byte field (lfgpu_sumcheck_layer)");
  LF_HIP(c, hipSetDevice(c->device));
  const F256 F;
  const E wi[2] = {e_of(wc_in[0]), e_of(wc_in[1])};
  E wo[2], bq;
  Tramp256 t{round, user};
  // the caller's arrays are words (8-byte aligned), the elements want 16: everything crosses the boundary by copy
  const std::vector<E> G0 = es_of(h_G0, logv), G1 = es_of(h_G1, logv);
  std::vector<E> g(2 * logw + 1);
  LF_TRY(sumcheck_layer256(q, F, logv, G0.data(), G1.data(), e_of(alpha), e_of(beta), logw, nw, (const E*)d_W, wi, tramp256_cb, &t, wo, g.data(), &bq));
  if (logw) memcpy(g_out, g.data(), 2 * logw * 32);
  memcpy(wc_out[0], wo[0].l, 32);
  memcpy(wc_out[1], wo[1].l, 32);
  if (bound_quad) memcpy(bound_quad, bq.l, 32);
  return LFGPU_OK;
}

extern "C" int lfgpu_sumcheck_layer_batch256(lfgpu_quad* q, size_t nb, size_t logv, const void* h_G0, const void* h_G1, const uint64_t* alpha,
                                             const uint64_t* beta, size_t logw, size_t nw, const void* d_W, size_t ldw, const uint64_t* wc_in,
                                             lfgpu_sc_round_batch256_fn round, void* user, uint64_t* wc_out, uint64_t* g_out, uint64_t* bound_quad) {
  if (!q) return LFGPU_ERR_ARG;
  lfgpu_ctx* c = q->c;
  if (!alpha || !beta || !d_W || !wc_in || !round || !wc_out || (logw && !g_out) || (logv && (!h_G0 || !h_G1)))
    return lf_fail(c, LFGPU_ERR_ARG, "sumcheck_layer_batch256: null argument");
  if (q->field != LFGPU_FIELD_P256) return lf_fail(c, LFGPU_ERR_ARG, "sumcheck_layer_batch256: the quad is over a 16-byte field (lfgpu_sumcheck_layer_batch)");
  if (nb == 0 || nb > LFGPU_SC_BATCH_MAX) return lf_fail(c, LFGPU_ERR_ARG, "sumcheck_layer_batch256: nb must be 1..%d", LFGPU_SC_BATCH_MAX);
  if (nw == 0 || logw > 40 || nw > ((size_t)1 << logw) || nw <= q->hmax)
    return lf_fail(c, LFGPU_ERR_ARG, "sumcheck_layer_batch256: nw = %zu must exceed the largest hand index %zu and fit 2^logw", nw, q->hmax);
  if (ldw < nw || ((ldw * nb) >> 40)) return lf_fail(c, LFGPU_ERR_ARG, "sumcheck_layer_batch256: ldw = %zu < nw = %zu", ldw, nw);
  if (logv > 40 || ((size_t)1 << logv) < q->nv) return lf_fail(c, LFGPU_ERR_ARG, "sumcheck_layer_batch256: 2^logv < nv");
  LF_HIP(c, hipSetDevice(c->device));
  const F256 F;
  static_assert(sizeof(E) == 32, "the ABI's [4] words are an element");
  const std::vector<E> G0 = es_of(h_G0, nb * logv), G1 = es_of(h_G1, nb * logv), al = es_of(alpha, nb), be = es_of(beta, nb), wi = es_of(wc_in, 2 * nb);
  std::vector<E> wo(2 * nb), g(2 * nb * logw + 1), bq(nb);
  LF_TRY(sumcheck_layer_batch256(q, F, nb, logv, G0.data(), G1.data(), al.data(), be.data(), logw, nw, (const E*)d_W, ldw, wi.data(), round, user, wo.data(),
                                 g.data(), bq.data()));
  memcpy(wc_out, wo.data(), 2 * nb * 32);
  if (logw) memcpy(g_out, g.data(), 2 * nb * logw * 32);
  if (bound_quad) memcpy(bound_quad, bq.data(), nb * 32);
  return LFGPU_OK;
}

int lf256_eval_quad_async(lfgpu_quad* q, const void* d_W, void* d_V, int* d_fail) {
  lfgpu_ctx* c = q->c;
  void* acc = nullptr;
  LF_TRY(lf_scratch2(c, q->nv * 64 + 64, &acc));
  LF_HIP(c, hipMemsetAsync(acc, 0, q->nv * 64, c->stream));
  hipLaunchKernelGGL(eval_quad256_kernel, dim3(nblk(q->n)), dim3(Z_THREADS), 0, c->stream, q->n, (const corner4*)q->d_bygate, (const E*)q->d_kvec, (const E*)d_W,
                     (u64*)acc, d_fail);
  hipLaunchKernelGGL(limb_normalize256_kernel, dim3(nblk(q->nv)), dim3(Z_THREADS), 0, c->stream, q->nv, (u64*)acc, h256_rsq(), (E*)d_V);
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}

// ProverLayers::eval_quad for nb statements of one quad: two launches whatever nb; 64 bytes of limb accumulators per output and
// statement, so no two statements share one.  Enqueue only: a violated assert-zero term of statement b ORs into d_fail[b], which
// the caller has cleared and reads back when it wants the verdict (zkp::prove_batch: once, after the last layer).
int lf256_eval_quad_batch_async(lfgpu_quad* q, size_t nb, const void* d_W, size_t ldw, void* d_V, size_t ldv, int* d_fail) {
  lfgpu_ctx* c = q->c;
  if ((q->nv * 64) > ((size_t)1 << 40) / nb) return lf_fail(c, LFGPU_ERR_NOMEM, "eval_quad_batch256: %zu bytes of accumulators per statement", q->nv * 64);
  void* acc = nullptr;
  LF_TRY(lf_scratch2(c, nb * q->nv * 64 + 64, &acc));
  LF_HIP(c, hipMemsetAsync(acc, 0, nb * q->nv * 64, c->stream));
  hipLaunchKernelGGL(eval_quad256_batch_kernel, dim3(nblk(q->n), (u32)nb), dim3(Z_THREADS), 0, c->stream, q->n, (const corner4*)q->d_bygate, (const E*)q->d_kvec,
                     (const E*)d_W, ldw, (u64*)acc, q->nv * 8, d_fail);
  hipLaunchKernelGGL(limb_normalize256_batch_kernel, dim3(nblk(q->nv), (u32)nb), dim3(Z_THREADS), 0, c->stream, q->nv, (u64*)acc, q->nv * 8, h256_rsq(), (E*)d_V, ldv);
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}

extern "C" int lfgpu_eval_quad_batch256(lfgpu_quad* q, size_t nb, size_t nw, const void* d_W, size_t ldw, void* d_V, size_t ldv, int* ok_out) {
  if (!q) return LFGPU_ERR_ARG;
  lfgpu_ctx* c = q->c;
  if (!d_W || !d_V || !ok_out) return lf_fail(c, LFGPU_ERR_ARG, "eval_quad_batch256: null argument");
  if (q->field != LFGPU_FIELD_P256) return lf_fail(c, LFGPU_ERR_ARG, "eval_quad_batch256: the quad is over a 16-byte field (lfgpu_eval_quad_batch)");
  if (nb == 0 || nb > LFGPU_SC_BATCH_MAX) return lf_fail(c, LFGPU_ERR_ARG, "eval_quad_batch256: nb must be 1..%d", LFGPU_SC_BATCH_MAX);
  if (nw <= q->hmax || ldw < nw || ldv < q->nv || ((ldw * nb) >> 40) || ((ldv * nb) >> 40))
    return lf_fail(c, LFGPU_ERR_ARG, "eval_quad_batch256: nw = %zu (a corner reads wire %zu), ldw = %zu, ldv = %zu (nv = %zu)", nw, q->hmax, ldw, ldv, q->nv);
  if ((q->nv * 64) > ((size_t)1 << 40) / nb) return lf_fail(c, LFGPU_ERR_NOMEM, "eval_quad_batch256: %zu bytes of accumulators per statement", q->nv * 64);
  LF_HIP(c, hipSetDevice(c->device));
  int* d_fail = (int*)((uint8_t*)c->mailbox_d + LF_EVALB_FAIL_OFF);
  LF_HIP(c, hipMemsetAsync(d_fail, 0, nb * 4, c->stream));
  LF_TRY(lf256_eval_quad_batch_async(q, nb, d_W, ldw, d_V, ldv, d_fail));
  LF_HIP(c, hipMemcpyAsync(c->mailbox_h, d_fail, nb * 4, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipStreamSynchronize(c->stream));
  for (size_t b = 0; b < nb; ++b) ok_out[b] = ((const int*)c->mailbox_h)[b] ? 0 : 1;
  return LFGPU_OK;
}

// ------------------------------------------------------------------ Ligero over 32-byte elements (one GPU holds all rows)
namespace {
// The width policy of ligero_slab.h for Fp256Base: the row kernels above, lfgpu_fp256_rs_encode_rows and lf_column_leaves32.  The
// prover is bound by a latency chain of short launches, so these steps only enqueue: host vectors go to lf_scratch2
// by plain asynchronous copies, and whoever reads the result back synchronises.  The one exception is a_rows_sparse.
// inner_product_vector's inputs for a_rows_terms (LfLigeroTerms of zkint.h over 32-byte elements), all on the host
struct Terms256 {
  const lfgpu_ligero_llterm256* term;
  size_t nterm;
  const E* alphal;  // [nl]
  size_t nl;
  const size_t* lqc;  // [nq][3]
  const E* alphaq;    // [nq][3]
};
struct L32 : lig::Host32 {
  static int rows_axpy(lfgpu_ctx* c, size_t nrows, size_t n, E* d_y, const E* h_u, const E* d_T, size_t ld) {
    void* du = nullptr;
    LF_TRY(lf_scratch2(c, nrows * 32 + 64, &du));
    LF_HIP(c, hipMemcpyAsync(du, h_u, nrows * 32, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(rows_axpy256_kernel, dim3(nblk(n, 64)), dim3(256), 0, c->stream, (u32)nrows, n, d_y, (const E*)du, d_T, ld);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  static int rows_vaxpy(lfgpu_ctx* c, size_t nrows, size_t n, const E* T0, const E* A, size_t lda, const E* T, size_t ld, E* y) {
    hipLaunchKernelGGL(rows_vaxpy256_kernel, dim3(nblk(n, 64)), dim3(256), 0, c->stream, (u32)nrows, n, T0, A, lda, T, ld, y);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  static int quad_combo(lfgpu_ctx* c, size_t nt, size_t n, const E* Tq, const E* u, const E* X, const E* Y, const E* Zr, size_t ld, E* y) {
    hipLaunchKernelGGL(quad_combo256_kernel, dim3(nblk(n)), dim3(Z_THREADS), 0, c->stream, (u32)nt, n, Tq, u, X, Y, Zr, ld, y);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  static int a_rows_clear(lfgpu_ctx*, E*, size_t, size_t, size_t) { return LFGPU_OK; }  // both callers clear the whole matrix themselves
  static int a_rows_dense(lfgpu_ctx* c, size_t r, size_t w, size_t ld, const E& scale, const E* d_dense, size_t n, E* d_rows) {
    hipLaunchKernelGGL(a_rows_dense256_kernel, dim3(nblk(n)), dim3(Z_THREADS), 0, c->stream, (u32)r, (u32)w, ld, scale, d_dense, n, d_rows);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  // (a_rows_sparse256_kernel has no bound on idx: lig::a_rows has checked the list against nflat on the host)
  static int a_rows_sparse(lfgpu_ctx* c, size_t r, size_t w, size_t ld, const uint64_t* h_idx, const E* h_val, size_t n, size_t /*nflat*/, E* d_rows) {
    void* d_sp = nullptr;
    LF_TRY(lf_scratch2(c, n * 40 + 64, &d_sp));
    E* d_val = (E*)d_sp;
    u64* d_idx = (u64*)(d_val + n);
    LF_HIP(c, hipMemcpyAsync(d_val, h_val, n * 32, hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipMemcpyAsync(d_idx, h_idx, n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(a_rows_sparse256_kernel, dim3(nblk(n)), dim3(Z_THREADS), 0, c->stream, (u32)r, (u32)w, ld, (const u64*)d_idx, (const E*)d_val, n, d_rows);
    LF_HIP(c, hipGetLastError());
    LF_HIP(c, hipStreamSynchronize(c->stream));  // the staging area is the Reed-Solomon encoder's work space next
    return LFGPU_OK;
  }
  // inner_product_vector from an unsorted term list with duplicates (a_terms256_kernel and its two companions), added to what
  // stands in the rows.  The accumulators, the term list (one copy, as the caller holds it) and the challenges (one packed copy)
  // live in scratch2, which is the Reed-Solomon encoder's work space next, and the term list is the caller's memory: this step
  // ends with a synchronise.  The caller has validated the statement (terms256_ok).
  static int a_rows_terms(lfgpu_ctx* c, const lfgpu_ligero_param& p, size_t ld, const Terms256& t, E* d_rows) {
    const size_t nflat = p.nwqrow * p.w, n3 = 3 * p.nq, acc_bytes = nflat * 64;
    const size_t small_bytes = (t.nl + n3) * 32 + n3 * 8;
    void* d = nullptr;
    LF_TRY(lf_scratch2(c, acc_bytes + t.nterm * 48 + small_bytes + 64, &d));
    u64* d_acc = (u64*)d;
    llterm256_t* d_term = (llterm256_t*)((uint8_t*)d + acc_bytes);
    E* d_alphal = (E*)(d_term + t.nterm);
    E* d_alphaq = d_alphal + t.nl;
    u64* d_lqc = (u64*)(d_alphaq + n3);
    LF_HIP(c, hipMemsetAsync(d_acc, 0, acc_bytes, c->stream));
    if (t.nterm) LF_HIP(c, hipMemcpyAsync(d_term, t.term, t.nterm * 48, hipMemcpyHostToDevice, c->stream));
    std::vector<uint8_t> pack(small_bytes);
    if (small_bytes) {
      if (t.nl) memcpy(pack.data(), t.alphal, t.nl * 32);
      if (n3) memcpy(pack.data() + t.nl * 32, t.alphaq, n3 * 32);
      if (n3) memcpy(pack.data() + (t.nl + n3) * 32, t.lqc, n3 * 8);
      LF_HIP(c, hipMemcpyAsync(d_alphal, pack.data(), small_bytes, hipMemcpyHostToDevice, c->stream));
    }
    auto run = [&]() -> int {
      if (t.nterm) {
        const dim3 grid((u32)std::min<size_t>((t.nterm + AT256_THREADS - 1) / AT256_THREADS, AT256_BLOCKS_MAX));
        hipLaunchKernelGGL(a_terms256_kernel, grid, dim3(AT256_THREADS), 0, c->stream, t.nterm, (const llterm256_t*)d_term, (const E*)d_alphal, d_acc);
      }
      if (n3)
        hipLaunchKernelGGL(a_terms_quad256_kernel, dim3(nblk(n3)), dim3(Z_THREADS), 0, c->stream, (u32)n3, (const u64*)d_lqc, (const E*)d_alphaq, (u64)(p.nwrow * p.w),
                           (u64)(p.nqtriples * p.w), d_acc);
      if (nflat)
        hipLaunchKernelGGL(a_terms_finish256_kernel, dim3(nblk(nflat)), dim3(Z_THREADS), 0, c->stream, (u32)p.r, (u32)p.w, ld, nflat, (const u64*)d_acc, h256_rsq(),
                           d_rows);
      LF_HIP(c, hipGetLastError());
      return LFGPU_OK;
    };
    const int rc = run();
    const hipError_t e = hipStreamSynchronize(c->stream);  // also after a failed launch: the copies out of `pack` and the caller's list may be pending
    if (rc) return rc;
    LF_HIP(c, e);
    return LFGPU_OK;
  }
  // h_idx is the caller's array and outlives the read-back that follows
  static int gather_columns(lfgpu_ctx* c, size_t nrow, size_t ld, size_t col0, const E* d_T, const size_t* h_idx, size_t nreq, E* d_req) {
    static_assert(sizeof(size_t) == sizeof(u64), "the kernel reads the indices as u64");
    void* di = nullptr;
    LF_TRY(lf_scratch2(c, nreq * 8 + 64, &di));
    LF_HIP(c, hipMemcpyAsync(di, h_idx, nreq * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(gather_columns256_kernel, dim3(nblk(nrow * nreq)), dim3(Z_THREADS), 0, c->stream, (u32)nrow, ld, col0, d_T, (const u64*)di, (u32)nreq, d_req);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  static int rs_rows(lfgpu_ctx* c, size_t nrow, size_t n, size_t m, E* d, size_t ld) { return lfgpu_fp256_rs_encode_rows(c, nrow, n, m, d, ld); }
  static int rs_rows_mixed(lfgpu_ctx*, size_t, size_t, size_t, size_t, size_t, size_t, E*, size_t) { return LFGPU_ERR_UNSUPPORTED; }  // group by group
  static int column_leaves(lfgpu_ctx* c, size_t nrow, size_t ld, size_t col0, size_t ncols, const void* d_T, const void* d_nonces, void* d_out) {
    return lf_column_leaves32(c, nrow, ld, col0, ncols, d_T, d_nonces, d_out, 0);
  }
  // ---- the steps of lig::prove_batch / open_batch over cb statements (the batch twins of the row kernels: statement blockIdx.y)
  // what the batch asks of 32-byte provers beyond lig::batch_core
  static int batch_ok(lfgpu_ctx* c, const char* who, lig::Slab<E>* const* pr, size_t nb, L32*) {
    for (size_t b = 0; b < nb; ++b) {
      if (pr[b]->sharded || !pr[b]->owns || pr[b]->row_lo != 0 || pr[b]->row_hi != pr[b]->p.nrow)
        return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "%s: prover %zu is sharded or holds a slab (the batch runs whole tableaux on one GPU)", who, b);
      if (!pr[b]->d_T) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu holds no commitment", who, b);
    }
    return LFGPU_OK;
  }
  // the encoder takes the rows of a chain in pairs: the pairs fit one launch's gridDim.y and their convolution scratch (64 bytes
  // per point) stays below the cap
  static size_t batch_rs_cap(const lfgpu_ligero_param& p) {
    if (!p.nwqrow) return SIZE_MAX;
    size_t P = 1;
    while (P < p.dblock) P <<= 1;
    return std::min<size_t>(2 * 65535 / p.nwqrow, LF_CB_SCRATCH_CAP / (((p.nwqrow + 1) / 2) * P * sizeof(fp2_t)));
  }
  static int a_rows_dense_batch(lfgpu_ctx* c, size_t cb, size_t r, size_t w, size_t ld, const E* d_scale, const LfBatchPtrs& dense, size_t n, E* d_rows, size_t srows) {
    hipLaunchKernelGGL(a_rows_dense256_batch_kernel, dim3(nblk(n), (u32)cb), dim3(Z_THREADS), 0, c->stream, (u32)r, (u32)w, ld, d_scale, dense, n, d_rows, srows);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  // (no bound on idx in the kernel: lig::prove_batch has checked every list against nflat on the host)
  static int a_rows_sparse_batch(lfgpu_ctx* c, size_t cb, size_t r, size_t w, size_t ld, const u64* d_idx, const E* d_val, const u64* d_off, size_t maxn,
                                 size_t /*nflat*/, E* d_rows, size_t srows) {
    hipLaunchKernelGGL(a_rows_sparse256_batch_kernel, dim3(nblk(maxn), (u32)cb), dim3(Z_THREADS), 0, c->stream, (u32)r, (u32)w, ld, d_idx, d_val, d_off, d_rows, srows);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  // the rows of all statements of the chain stand contiguously at the stride ld (srows = nrow * ld), so this is ONE extension of
  // cb * nrow rows (exact arithmetic: how the encoder pairs the rows does not change a value)
  static int rs_rows_batch(lfgpu_ctx* c, size_t cb, E* d_rows, size_t /*srows*/, size_t nrow, size_t n, size_t m, size_t ld) {
    return lfgpu_fp256_rs_encode_rows(c, cb * nrow, n, m, d_rows, ld);
  }
  // dot proof (dblock columns) into y_b + block, low-degree proof (block columns) into y_b
  static int rows_combo_batch(lfgpu_ctx* c, size_t cb, const lfgpu_ligero_param& p, const LfBatchPtrs& T, const E* A, size_t sA, const E* u, E* y, size_t sy) {
    const size_t ld = p.block_enc;
    hipLaunchKernelGGL(rows_vaxpy256_batch_kernel, dim3(nblk(p.dblock, 64), (u32)cb), dim3(256), 0, c->stream, (u32)p.nwqrow, p.dblock, T, ld, p.idot * ld, p.iw * ld, A, sA,
                       p.dblock, y + p.block, sy);
    hipLaunchKernelGGL(rows_axpy256_batch_kernel, dim3(nblk(p.block, 64), (u32)cb), dim3(256), 0, c->stream, (u32)p.nwqrow, p.block, T, ld, p.ildt * ld, p.iw * ld, u,
                       p.nwqrow, y, sy);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  static int quad_combo_batch(lfgpu_ctx* c, size_t cb, const lfgpu_ligero_param& p, const LfBatchPtrs& T, const E* u, E* y, size_t sy) {
    const size_t ld = p.block_enc;
    hipLaunchKernelGGL(quad_combo256_batch_kernel, dim3(nblk(p.dblock), (u32)cb), dim3(Z_THREADS), 0, c->stream, (u32)p.nqtriples, p.dblock, T, ld, p.iquad * ld, p.iq * ld,
                       u, p.nqtriples, y, sy);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  static int gather_columns_batch(lfgpu_ctx* c, size_t cb, size_t nrow, size_t ld, size_t col0, const LfBatchPtrs& T, const u64* d_idx, size_t nreq, E* d_req) {
    hipLaunchKernelGGL(gather_columns256_batch_kernel, dim3(nblk(nrow * nreq), (u32)cb), dim3(Z_THREADS), 0, c->stream, (u32)nrow, ld, col0, T, d_idx, (u32)nreq, d_req);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
};
using Lig32 = lig::Slab<E>;  // the prover record: all rows on one GPU, or a slab with a communicator (lfgpu_zk_prover_set_comm above the size threshold)

// cm != nullptr (more than one rank; the caller has made every rank's `rng` yield the same bytes): every rank consumes the whole
// stream and lays out, keeps and encodes its own row slab (lig::layout), and the columns are committed as in
// lfgpu_ligero_commit_sharded (lig::commit_rows)
int lig256_commit(lfgpu_ctx* c, const lfgpu_ligero_param& p, const E* W, const size_t* lqc, lfgpu_rng_fn rng, void* user, uint8_t root[32], Lig32** out,
                  const lfgpu_comm_ops* cm = nullptr) {
  if (p.ildt != 0 || p.idot != 1 || p.iquad != 2 || p.iw != 3) return lf_fail(c, LFGPU_ERR_ARG, "ligero256: row order");
  const double t0 = lig::clock_ms();
  std::unique_ptr<Lig32> L(new Lig32());
  L->init(c, p, cm);
  std::vector<E> H(std::max<size_t>(L->row_hi - L->row_lo, 1) * p.dblock);
  LF_SCRUB_ON_EXIT(H);
  char err[256] = {0};
  const int rc = lig::layout(L32(), p, W, 0, lqc, rng, user, c->rng_exact != 0, L->row_lo, L->row_hi, H.data(), L->nonces.data(), err);
  if (rc) return lf_fail(c, rc, "%s", err);
  LF_TRY(lig::commit_rows(L.get(), L32(), H.data(), t0, root));
  *out = L.release();
  return LFGPU_OK;
}
Lig32* lig32_of(Lig256* L) { return reinterpret_cast<Lig32*>(L); }

// ---- nb commits of one shape in one chain of dispatches (lfgpu_ligero_commit_batch256, zk256_commit_batch): what
// lfgpu_ligero_commit_batch is for the 16-byte fields.  A single commit is a chain of short launches -- three row groups, each
// pre, forward transform, pointwise product, inverse transform, post; then leaves and tree -- over a tableau of a few MB, so nb
// provers pay the chain nb times.  Here the rows [0, idot) and [iquad + 1, nrow) of every statement of a chunk (all encode
// `block` values with the same tables) go through ONE chain, the two dblock rows of every statement through a second, and the
// leaves and trees of all statements follow (lfgpu_column_commit_batch256).
// Statements per chain: the row pairs of the larger group fit one launch's gridDim.y and their convolution scratch stays below
// LF_CB_SCRATCH_CAP; LFGPU_CB_CHUNK overrides (read once).  0: not even one statement fits -- the single path's encoder.
size_t commit_batch256_chunk(const lfgpu_ligero_param& p, size_t nb) {
  static const long env = getenv("LFGPU_CB_CHUNK") ? atol(getenv("LFGPU_CB_CHUNK")) : 0;
  const size_t rows = std::max<size_t>(p.nrow - 2, 2);
  size_t P = 1;
  while (P < p.block_enc) P <<= 1;
  const size_t pairs_max = std::min<size_t>(65535, LF_CB_SCRATCH_CAP / (P * sizeof(fp2_t)));
  size_t chunk = std::min(nb, 2 * pairs_max / rows);
  if (env > 0) chunk = std::min(chunk, (size_t)env);
  return chunk;
}
// W[b]: witness || pads of statement b; users may be null.  On success out[b] is statement b's prover and roots[32 b ..] its root;
// on any error no prover is returned.  Draws, staging and errors: the contract of lfgpu_ligero_commit_batch256 (lfgpu.h).
int lig256_commit_batch(lfgpu_ctx* c, const lfgpu_ligero_param& p, size_t nb, const E* const* W, const size_t* lqc, const lfgpu_rng_fn* rng, void* const* users,
                        uint8_t* roots, Lig32** out) {
  static const char* const who = "ligero_commit_batch256";
  if (p.ildt != 0 || p.idot != 1 || p.iquad != 2 || p.iw != 3 || p.nrow < 3) return lf_fail(c, LFGPU_ERR_ARG, "ligero256: row order");
  for (size_t b = 0; b < nb; ++b) out[b] = nullptr;
  auto user = [&](size_t b) { return users ? users[b] : nullptr; };
  auto drop = [&](int rc) {  // no prover is returned: their buffers go back to the pool scrubbed (~Slab)
    for (size_t b = 0; b < nb; ++b) {
      delete out[b];
      out[b] = nullptr;
    }
    return rc;
  };
  static const int batched = getenv("LFGPU_COMMIT_BATCH256") ? atoi(getenv("LFGPU_COMMIT_BATCH256")) : 1;
  if (!batched) {  // the A/B switch: the same semantics over the single-statement device path
    for (size_t b = 0; b < nb; ++b) {
      const int rc = lig256_commit(c, p, W[b], lqc, rng[b], user(b), roots + 32 * b, &out[b]);
      if (rc) return drop(rc);
    }
    return LFGPU_OK;
  }
  const size_t ld = p.block_enc, hw = p.dblock, ncols = p.block_ext;
  LF_HIP(c, hipSetDevice(c->device));
  static const bool verbose = getenv("LFGPU_VERBOSE") != nullptr;
  const double tv0 = lig::clock_ms();
  // pinned staging: [nb][nrow][dblock] un-encoded images, then [nb][ncols][32] nonces
  const size_t img = p.nrow * hw * sizeof(E), used = nb * (img + ncols * 32);
  uint8_t* stage = nullptr;
  LF_TRY(lig::cb_stage(c, who, used, &stage));
  uint8_t* const h_non = stage + nb * img;
  const lig::CbScrub scrub{stage, used};
  // the host half, statement by statement in index order: all draws of statement b from rng[b]
  for (size_t b = 0; b < nb; ++b) {
    char err[256] = {0};
    const int rc = lig::layout(L32(), p, W[b], 0, lqc, rng[b], user(b), c->rng_exact != 0, 0, p.nrow, (E*)(stage + b * img), h_non + b * ncols * 32, err);
    if (rc) return lf_fail(c, rc, "%s (statement %zu)", err, b);
  }
  const double tv1 = lig::clock_ms();
  // Everything that may synchronise comes before the first enqueue: the encoder's tables of both shapes (first use: synchronous
  // copies and a synchronise) and the growth of the scratch slots.  The slots of the chain: the convolution scratch Z is scratch2,
  // the nonces scratch3, the roots scratch (lfgpu_column_commit_batch256); the tableaux and heaps are the provers' own.
  const size_t chunk = commit_batch256_chunk(p, nb), g1 = p.nrow - 2;
  void *d_Z = nullptr, *d_non = nullptr, *d_roots = nullptr;
  if (chunk) {
    LF_TRY(lf_p256_rs_prepare(c, p.block, p.block_enc));
    LF_TRY(lf_p256_rs_prepare(c, p.dblock, p.block_enc));
    LF_TRY(lf_scratch2(c, lf_p256_rs_batch_scratch(chunk * std::max<size_t>(g1, 2), p.block_enc), &d_Z));
  }
  LF_TRY(lf_scratch3(c, nb * ncols * 32, &d_non));
  LF_TRY(lf_scratch(c, LFGPU_SC_BATCH_MAX * 32, &d_roots));
  // After a failed enqueue the stream may still read the staging memory: wait before it is scrubbed
  auto fail = [&](int rc) {
    (void)hipStreamSynchronize(c->stream);
    return drop(rc);
  };
  E* d_T[LFGPU_SC_BATCH_MAX];
  void* d_L[LFGPU_SC_BATCH_MAX];
  int rc = LFGPU_OK;
  for (size_t b = 0; b < nb; ++b) {
    Lig32* L = out[b] = new Lig32();
    L->init(c, p, nullptr);
    L->nonces.assign(h_non + b * ncols * 32, h_non + (b + 1) * ncols * 32);
    if ((rc = L->alloc())) return fail(rc);
    d_T[b] = L->d_T;
    d_L[b] = L->d_layers;
  }
  for (size_t b = 0; b < nb; ++b)
    if (hipMemcpy2DAsync(d_T[b], ld * sizeof(E), stage + b * img, hw * sizeof(E), hw * sizeof(E), p.nrow, hipMemcpyHostToDevice, c->stream) != hipSuccess)
      return fail(lf_fail(c, LFGPU_ERR_HIP, "%s: upload failed (statement %zu)", who, b));
  for (size_t b0 = 0; b0 < nb; b0 += std::max<size_t>(chunk, 1)) {
    if (!chunk) {  // a row group of one statement overflows a launch or the cap: the single path's encoder
      if ((rc = lig::extend_slab(c, L32(), p, 0, p.nrow, d_T[b0]))) return fail(rc);
      continue;
    }
    const size_t cb = std::min(chunk, nb - b0);
    LfBatchPtrs pt{};
    for (size_t b = 0; b < cb; ++b) pt.p[b] = d_T[b0 + b];
    if ((rc = lf_p256_rs_rows_batch(c, cb, pt, 0, p.idot, 2, g1, p.block, p.block_enc, ld, d_Z))) return fail(rc);   // [0, idot) + [iquad + 1, nrow)
    if ((rc = lf_p256_rs_rows_batch(c, cb, pt, p.idot, 2, 0, 2, p.dblock, p.block_enc, ld, d_Z))) return fail(rc);  // idot, iquad
  }
  // the nonces go up behind the encode, as in lig::commit_rows
  if (hipMemcpyAsync(d_non, h_non, nb * ncols * 32, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    return fail(lf_fail(c, LFGPU_ERR_HIP, "%s: nonce upload failed", who));
  double tv2 = 0;
  if (verbose) {
    (void)hipStreamSynchronize(c->stream);
    tv2 = lig::clock_ms();
  }
  // (ends with the one stream synchronise of the call: the uploads above are over when it returns)
  if ((rc = lfgpu_column_commit_batch256(c, p.nrow, ld, p.dblock, ncols, nb, (const void* const*)d_T, d_non, d_L, roots))) return fail(rc);
  if (verbose)
    fprintf(stderr, "lfgpu ligero_commit_batch256: %zu x %zu rows x %zu (block %zu, dblock %zu): host layout + draws %.2f ms | upload + RS encode %.2f | column hash + tree %.2f\n",
            nb, p.nrow, ld, p.block, p.dblock, tv1 - tv0, tv2 - tv1, lig::clock_ms() - tv2);
  return LFGPU_OK;
}

// ---- lfgpu_ligero_prove_batch256 / lfgpu_ligero_open_batch256 (lfgpu.h): the provers of lfgpu_ligero_commit(field = P256) through
// lig::prove_batch / lig::open_batch (ligero_slab.h), which the ZK driver calls on its Lig32 directly (P32).
// The records behind the handles.  The range of nb and a NULL entry are lig::batch_core's to refuse: the conversion stops there.
int lig256_handles(lfgpu_ctx* c, const char* who, lfgpu_ligero_prover* const* pr, size_t nb, Lig32** out) {
  for (size_t b = 0; b < (nb <= LFGPU_SC_BATCH_MAX ? nb : 0) && pr[b]; ++b) {
    LfLigeroView v;
    lf_ligero_prover_view(pr[b], &v);
    if (v.c != c) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu belongs to another context", who, b);
    if (!v.lig256) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu is over a 16-byte field (lfgpu_ligero_prove_batch / lfgpu_ligero_open_batch serve those)", who, b);
    out[b] = lig32_of(v.lig256);
  }
  return LFGPU_OK;
}
}  // namespace
extern "C" int lfgpu_ligero_prove_batch256(lfgpu_ctx* c, lfgpu_ligero_prover* const* pr, size_t nb, const void* h_u_ldt, const void* const* d_dense, size_t ndense,
                                           const uint64_t* scale, const uint64_t* const* h_idx, const void* const* h_val, const size_t* nsparse,
                                           const void* h_u_quad, void* h_y_ldt, void* h_y_dot, void* h_y_q0, void* h_y_q2) {
  static const char* const who = "ligero_prove_batch256";
  if (!c || !pr || !nsparse || !h_y_ldt || !h_y_dot || !h_y_q0 || !h_y_q2) return lf_fail(c, LFGPU_ERR_ARG, "%s: null argument", who);
  Lig32* L[LFGPU_SC_BATCH_MAX] = {};
  LF_TRY(lig256_handles(c, who, pr, nb, L));
  return lig::prove_batch<L32>(c, who, L, nb, h_u_ldt, d_dense, ndense, scale, h_idx, h_val, nsparse, h_u_quad, h_y_ldt, h_y_dot, h_y_q0, h_y_q2);
}
extern "C" int lfgpu_ligero_open_batch256(lfgpu_ctx* c, lfgpu_ligero_prover* const* pr, size_t nb, const size_t* idx, void* h_req, uint8_t* h_nonces, uint8_t* h_path,
                                          size_t path_cap, size_t* npath) {
  static const char* const who = "ligero_open_batch256";
  if (!c || !pr || !idx || !h_req || !h_nonces || !npath) return lf_fail(c, LFGPU_ERR_ARG, "%s: null argument", who);
  Lig32* L[LFGPU_SC_BATCH_MAX] = {};
  LF_TRY(lig256_handles(c, who, pr, nb, L));
  return lig::open_batch<L32>(c, who, L, nb, idx, h_req, h_nonces, h_path, path_cap, npath);
}

// ---- behind lfgpu_ligero_commit / low_degree_proof / dot_proof / quadratic_proof / open / tableau / free for field P256
// (ligero.hip; declared in zkint.h): one GPU, all rows
int lf_lig256_commit(lfgpu_ctx* c, const lfgpu_ligero_param* p, const void* h_W, const size_t* h_lqc, lfgpu_rng_fn rng, void* user, uint8_t root[32], Lig256** out) {
  Lig32* L = nullptr;
  LF_TRY(lig256_commit(c, *p, (const E*)h_W, h_lqc, rng, user, root, &L));
  *out = reinterpret_cast<Lig256*>(L);
  return LFGPU_OK;
}
int lf_lig256_commit_batch(lfgpu_ctx* c, const lfgpu_ligero_param* p, size_t nb, const void* const* h_W, const size_t* h_lqc, const lfgpu_rng_fn* rng,
                           void* const* rng_user, uint8_t* roots, Lig256** out) {
  Lig32* L[LFGPU_SC_BATCH_MAX] = {};
  const int rc = lig256_commit_batch(c, *p, nb, (const E* const*)h_W, h_lqc, rng, rng_user, roots, L);
  for (size_t b = 0; b < nb; ++b) out[b] = reinterpret_cast<Lig256*>(L[b]);
  return rc;
}
void lf_lig256_free(Lig256* L) { delete lig32_of(L); }  // ~Slab scrubs the buffers and returns them to the context's pool
void* lf_lig256_tableau(Lig256* L) { return lig32_of(L)->d_T; }
int lf_lig256_low_degree(Lig256* L, const void* h_u, void* h_y) { return lig::low_degree(lig32_of(L), L32(), (const E*)h_u, (E*)h_y); }
// dot_proof (:293-309) with the caller's dense A (nwqrow x w, host): layout_Aext (ligero_param.h:423-430) is one strided copy
int lf_lig256_dot_dense(Lig256* L, const void* h_A, void* h_y) {
  Lig32* pr = lig32_of(L);
  lfgpu_ctx* c = pr->c;
  const lfgpu_ligero_param& p = pr->p;
  const size_t lda = p.dblock;
  void* sc = nullptr;
  LF_TRY(lf_scratch3(c, (p.nwqrow * p.w + p.nwqrow * lda + 2 * p.dblock) * 32 + 64, &sc));
  E* dA = (E*)sc;
  E* dAext = dA + p.nwqrow * p.w;
  E* dy = dAext + p.nwqrow * lda;
  LF_HIP(c, hipMemcpyAsync(dA, h_A, p.nwqrow * p.w * 32, hipMemcpyHostToDevice, c->stream));
  LF_HIP(c, hipMemsetAsync(dAext, 0, p.nwqrow * lda * 32, c->stream));
  if (p.nwqrow) LF_HIP(c, hipMemcpy2DAsync(dAext + p.r, lda * 32, dA, p.w * 32, p.w * 32, p.nwqrow, hipMemcpyDeviceToDevice, c->stream));
  LF_HIP(c, hipStreamSynchronize(c->stream));  // h_A is the caller's: its upload is over before the first error return below
  return lig::dot_finish(pr, L32(), dAext, dy, (E*)h_y);
}
int lf_lig256_quadratic(Lig256* L, const void* h_u, void* h_y0, void* h_y2) { return lig::quadratic(lig32_of(L), L32(), (const E*)h_u, (E*)h_y0, (E*)h_y2); }
int lf_lig256_open(Lig256* L, const size_t* idx, void* h_req, uint8_t* h_nonces, uint8_t* h_path, size_t path_cap, size_t* npath) {
  return lig::open(lig32_of(L), L32(), idx, (E*)h_req, h_nonces, h_path, path_cap, npath);
}
int lf_lig256_a_rows_terms(lfgpu_ctx* c, const lfgpu_ligero_param* p, size_t ld, const lfgpu_ligero_llterm256* term, size_t nterm, const void* h_alphal, size_t nl,
                           const size_t* h_lqc, const void* h_alphaq, void* d_rows) {
  const Terms256 t{term, nterm, (const E*)h_alphal, nl, h_lqc, (const E*)h_alphaq};
  return L32::a_rows_terms(c, *p, ld, t, (E*)d_rows);
}
int lf_lig256_a_rows_sparse(lfgpu_ctx* c, const lfgpu_ligero_param* p, size_t ld, const uint64_t* h_idx, const void* h_val, size_t n, void* d_rows) {
  return lig::a_rows(c, L32(), p->w, p->r, ld, p->nwqrow, (const E*)nullptr, 0, e32_zero(), h_idx, (const E*)h_val, n, (E*)d_rows);
}

// ------------------------------------------------------------------ the Fp256Base policy
namespace {
int bind_gh_all256(lfgpu_quad* q, const F256& F, size_t logv, const E* G0, const E* G1, const E& alpha, const E& beta, size_t logw, size_t nw, const E* H0,
                   const E* H1, E* out) {
  lfgpu_ctx* c = q->c;
  if (logv > 40 || logw > 40 || ((size_t)1 << logv) < q->nv || nw == 0 || ((size_t)1 << logw) < nw || nw <= q->hmax)
    return lf_fail(c, LFGPU_ERR_ARG, "bind_gh_all256: table sizes (nw must exceed the largest hand index %zu)", q->hmax);
  void* sc = nullptr;
  LF_TRY(lf_scratch3(c, (q->nv + 2 * nw) * 32 + 128, &sc));
  E* d_eqg = (E*)sc;
  E* d_eqh0 = d_eqg + q->nv;
  E* d_eqh1 = d_eqh0 + nw;
  u64* d_acc = (u64*)(d_eqh1 + nw);
  LF_TRY(raw_eq2_256(c, F, logv, q->nv, G0, G1, alpha, d_eqg));
  LF_TRY(raw_eq2_256(c, F, logw, nw, H0, H0, F.zero, d_eqh0));  // EQ(H0, i) + 0 * (...)
  LF_TRY(raw_eq2_256(c, F, logw, nw, H1, H1, F.zero, d_eqh1));
  LF_HIP(c, hipMemsetAsync(d_acc, 0, 64, c->stream));
  hipLaunchKernelGGL(bind_gh_all256_kernel, dim3(std::min<u32>(nblk(q->n), 1024)), dim3(Z_THREADS), 0, c->stream, q->n, (const corner4*)q->d_morton,
                     (const E*)q->d_kvec, (const E*)d_eqg, (const E*)d_eqh0, (const E*)d_eqh1, beta, d_acc);
  LF_HIP(c, hipGetLastError());
  u64 w[8];
  LF_TRY(lfgpu_memcpy_d2h(c, w, d_acc, 64));
  *out = fp256_reduce_limbs(w, F.rsq);
  return LFGPU_OK;
}

// Wire32 (zk_proto.h) plus the device steps of this file
struct P32 : zkp::Wire32 {
  using Lig = Lig32;
  using Layer = lfgpu_circuit::Layer;
  static constexpr const char* kProveName = "zk256_prove";
  static const F256& host_field(lfgpu_ctx*) {  // (the constants are built once)
    static const F256 F;
    return F;
  }
  static constexpr bool kDeferGh = false;  // Quad::bind_gh_all synchronises per layer
  static int eval_layer(lfgpu_quad* q, const void* d_W, void* d_V, int* d_fail) { return lf256_eval_quad_async(q, d_W, d_V, d_fail); }
  static int sumcheck_layer(lfgpu_quad* q, const F256& F, size_t logv, const E* G0, const E* G1, const E& alpha, const E& beta, size_t logw, size_t nw,
                            void* d_W, const E wc_in[2], round256_fn round, void* user, E wc_out[2], E* g_out, E* bound_quad) {
    return sumcheck_layer256(q, F, logv, G0, G1, alpha, beta, logw, nw, (const E*)d_W, wc_in, round, user, wc_out, g_out, bound_quad);
  }
  static int bind_gh_all(lfgpu_ctx*, const F256& F, const Layer& L, size_t logv, const E* G0, const E* G1, const E& alpha, const E& beta, const E* H0,
                         const E* H1, E* out) {
    return bind_gh_all256(L.q, F, logv, G0, G1, alpha, beta, L.logw, L.nw, H0, H1, out);
  }
  // EQ(H0, i) + alpha EQ(H1, i), i < n, into d_eq; its first npub entries back to the host
  static int eq_table(lfgpu_ctx* c, const F256& F, size_t logn, size_t n, const E* H0, const E* H1, const E& alpha, E* d_eq, size_t npub, E* eq_in) {
    LF_TRY(raw_eq2_256(c, F, logn, n, H0, H1, alpha, d_eq));
    if (npub) LF_TRY(lfgpu_memcpy_d2h(c, eq_in, d_eq, npub * 32));
    return LFGPU_OK;
  }
  // ---- the batch axis (zkp::prove_batch): B statements of one layer per call
  typedef void (*round_batch_fn)(void* user, size_t hand, size_t rnd, size_t nb, const E (*ev)[3], E* chal);
  static constexpr const char* kProveBatchName = "zk_prove_batch256";
  // LFGPU_LIGERO_PROVE_BATCH256 [1] (read once per process): 0 = constraints, Ligero prove and opening per statement (prove_finish)
  static int ligero_batch_switch() {
    static const int on = getenv("LFGPU_LIGERO_PROVE_BATCH256") ? atoi(getenv("LFGPU_LIGERO_PROVE_BATCH256")) : 1;
    return on;
  }
  static int eval_layer_batch(lfgpu_quad* q, size_t nb, const void* d_W, size_t ldw, void* d_V, size_t ldv, int* d_fail) {
    return lf256_eval_quad_batch_async(q, nb, d_W, ldw, d_V, ldv, d_fail);
  }
  // sumcheck_layer_batch256 spells its callback's elements as words: the template's callback is reached through a copy
  struct TrampBatch {
    round_batch_fn f;
    void* user;
    std::vector<E> ev, ch;
  };
  static void tramp_batch_cb(void* user, size_t hand, size_t rnd, size_t nb, const uint64_t (*ev)[3][4], uint64_t (*chal)[4]) {
    TrampBatch* t = (TrampBatch*)user;
    memcpy((void*)t->ev.data(), ev, nb * 96);
    t->f(t->user, hand, rnd, nb, (const E(*)[3])t->ev.data(), t->ch.data());
    memcpy(chal, t->ch.data(), nb * 32);
  }
  // G0 / G1: [nb][logv]; alpha, beta, bound_quad: [nb]; wc_in, wc_out: [nb][2]; g_out: [nb][2][logw]; d_W: statement b at b * ldw
  static int sumcheck_layer_batch(lfgpu_quad* q, const F256& F, size_t nb, size_t logv, const E* G0, const E* G1, const E* alpha, const E* beta, size_t logw,
                                  size_t nw, void* d_W, size_t ldw, const E* wc_in, round_batch_fn round, void* user, E* wc_out, E* g_out, E* bound_quad) {
    lfgpu_ctx* c = q->c;
    if (nw == 0 || logw > 40 || nw > ((size_t)1 << logw) || nw <= q->hmax || ldw < nw)  // (as sumcheck_layer256 and the kernel ABI check)
      return lf_fail(c, LFGPU_ERR_ARG, "zk_prove_batch256: nw must exceed the largest hand index and fit 2^logw and ldw");
    if (logv > 40 || ((size_t)1 << logv) < q->nv) return lf_fail(c, LFGPU_ERR_ARG, "zk_prove_batch256: 2^logv < nv");
    TrampBatch t{round, user, std::vector<E>(3 * nb), std::vector<E>(nb)};
    return sumcheck_layer_batch256(q, F, nb, logv, G0, G1, alpha, beta, logw, nw, (const E*)d_W, ldw, wc_in, tramp_batch_cb, &t, wc_out, g_out, bound_quad);
  }
  // eq_table for nb statements in one upload and one launch chain: H0 / H1 [nb][logn], statement b's table at d_eq + b * n, its
  // first npub entries to eq_in + b * npub in ONE read-back
  static int eq_table_batch(lfgpu_ctx* c, const F256& F, size_t nb, size_t logn, size_t n, const E* H0, const E* H1, const E* alpha, E* d_eq, size_t npub,
                            E* eq_in) {
    const std::vector<E> no_beta(nb, e32_zero());  // the table's beta slot is bind_g's
    const E* d_pts = nullptr;
    LF_TRY(raw_eq2_256_batch(c, F, nb, logn, n, H0, H1, alpha, no_beta.data(), d_eq, &d_pts));
    if (npub) {  // (without public inputs nothing is read: the tables are consumed in stream order by the dot proofs)
      LF_HIP(c, hipMemcpy2DAsync(eq_in, npub * 32, d_eq, n * 32, npub * 32, nb, hipMemcpyDeviceToHost, c->stream));
      LF_HIP(c, hipStreamSynchronize(c->stream));
    }
    return LFGPU_OK;
  }
  static int ligero_prove_batch(lfgpu_ctx* c, Lig* const* lp, size_t nb, const E* u_ldt, const E* const* d_dense, size_t ndense, const E* scale,
                                const uint64_t* const* idx, const E* const* val, const size_t* nsparse, const E* u_quad, E* y_ldt, E* y_dot, E* y_q0, E* y_q2) {
    return lig::prove_batch<L32>(c, kProveBatchName, lp, nb, u_ldt, (const void* const*)d_dense, ndense, scale, idx, (const void* const*)val, nsparse, u_quad, y_ldt,
                                 y_dot, y_q0, y_q2);
  }
  static int ligero_open_batch(lfgpu_ctx* c, Lig* const* lp, size_t nb, const size_t* idx, E* req, uint8_t* nonces, uint8_t* path, size_t cap, size_t* npath) {
    return lig::open_batch<L32>(c, kProveBatchName, lp, nb, idx, req, nonces, path, cap, npath);
  }
  static int low_degree(Lig* lp, const E* u, E* y) { return lig::low_degree(lp, L32(), u, y); }
  static int dot(Lig* lp, const E* d_dense, size_t ndense, const E& scale, const uint64_t* idx, const E* val, size_t nsparse, E* y) {
    return lig::dot(lp, L32(), d_dense, ndense, scale, idx, val, nsparse, y);
  }
  static int quadratic(Lig* lp, const E* u, E* y0, E* y2) { return lig::quadratic(lp, L32(), u, y0, y2); }
  static int open(Lig* lp, const size_t* idx, E* req, uint8_t* nonces, uint8_t* path, size_t cap, size_t* npath) {
    return lig::open(lp, L32(), idx, req, nonces, path, cap, npath);
  }
  static size_t verifier_bytes(const lfgpu_circuit_info& I, const lfgpu_ligero_param& p) {
    return (I.ninputs + (p.nwqrow + 3) * p.block_enc + (p.nwqrow + 3) * p.nreq) * 32 + 256;
  }
  // LigeroVerifier: rows [0, nwqrow) = [0^r | A_i] (inner_product_vector + layout_Aext), then y_ldt, y_dot, y_quad, extended
  // to block_enc; ext = those rows at the opened columns.  The verifier's device buffer (lf_scratch4, verifier_bytes) is
  // EQ table of the input constraint | the rows | the gathered columns.
  static int verifier_ext(lfgpu_ctx* c, const F256&, const lfgpu_circuit_info& I, const lfgpu_ligero_param& p, const E* d_eq, const E& scale,
                          const std::vector<uint64_t>& a_idx, const std::vector<E>& a_val, const zkp::ProofBody<E>& pr, const size_t* idx, std::vector<E>& ext) {
    const size_t n_witness = I.ninputs - I.npub_in;
    auto a_rows = [&](E* d_T, size_t ld) {
      return lig::a_rows(c, L32(), p.w, p.r, ld, p.nwqrow, d_eq + I.npub_in, n_witness, scale, a_idx.data(), a_val.data(), a_idx.size(), d_T);
    };
    return verifier_ext_with(c, p, (E*)d_eq + I.ninputs, a_rows, pr, idx, ext);
  }
  // ... with the A rows from the caller's step a_rows(d_T, ld) (ZkVerifier above; lfgpu_ligero_verify256: the term list), in
  // d_T: room for (nwqrow + 3) * (block_enc + nreq) elements
  template <class ARows>
  static int verifier_ext_with(lfgpu_ctx* c, const lfgpu_ligero_param& p, E* d_T, ARows a_rows, const zkp::ComProof<E>& pr, const size_t* idx, std::vector<E>& ext) {
    const size_t nrows_dev = p.nwqrow + 3, ld = p.block_enc;
    E* d_req = d_T + nrows_dev * ld;
    LF_HIP(c, hipMemset2DAsync(d_T, ld * 32, 0, p.dblock * 32, nrows_dev, c->stream));
    LF_TRY(a_rows(d_T, ld));
    LF_HIP(c, hipMemcpyAsync(d_T + (p.nwqrow + 0) * ld, pr.y_ldt.data(), p.block * 32, hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipMemcpyAsync(d_T + (p.nwqrow + 1) * ld, pr.y_dot.data(), p.dblock * 32, hipMemcpyHostToDevice, c->stream));
    E* yq = d_T + (p.nwqrow + 2) * ld;  // y_quad = y_quad_0 | 0^w | y_quad_2
    LF_HIP(c, hipMemcpyAsync(yq, pr.y_q0.data(), p.r * 32, hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipMemcpyAsync(yq + p.block, pr.y_q2.data(), (p.dblock - p.block) * 32, hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));  // the staging area is the Reed-Solomon encoder's work space next
    LF_TRY(lfgpu_fp256_rs_encode_rows(c, p.nwqrow + 1, p.block, p.block_enc, d_T, ld));             // A rows and y_ldt
    LF_TRY(lfgpu_fp256_rs_encode_rows(c, 2, p.dblock, p.block_enc, d_T + (p.nwqrow + 1) * ld, ld));  // y_dot, y_quad
    void* di = nullptr;
    LF_TRY(lf_scratch2(c, p.nreq * 8 + 64, &di));
    std::vector<u64> ix(idx, idx + p.nreq);
    LF_HIP(c, hipMemcpyAsync(di, ix.data(), p.nreq * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(gather_columns256_kernel, dim3(nblk(nrows_dev * p.nreq)), dim3(Z_THREADS), 0, c->stream, (u32)nrows_dev, ld, p.dblock, (const E*)d_T,
                       (const u64*)di, (u32)p.nreq, d_req);
    LF_HIP(c, hipGetLastError());
    LF_HIP(c, hipStreamSynchronize(c->stream));
    ext.resize(nrows_dev * p.nreq);
    return lfgpu_memcpy_d2h(c, ext.data(), d_req, ext.size() * 32);
  }
  // ---- the driver layer (zk_driver.h)
  static constexpr const char *kName = "zk256", *kCommitName = "zk256_commit", *kCommitBatchName = "zk_commit_batch256", *kBatchNewName = "zk_batch256_new";
  static constexpr int kLigeroK = 0;
  struct ProverExtra {
    // the prover's own EQ table of the input constraint: a function of the challenges only, cleared with the prover's other
    // buffers all the same
    void* d_eq = nullptr;
    int init(lfgpu_ctx* c, int, int, size_t ninputs, zkp::Owned* mem) {
      if (mem && !mem->alloc(&d_eq, ninputs * 32, true)) return lf_fail(c, LFGPU_ERR_NOMEM, "zk256: EQ table over the inputs");
      return LFGPU_OK;
    }
  };
  static P32 make(lfgpu_ctx*, int, int, const ProverExtra*) { return P32(); }
  static int ts_ok(lfgpu_ctx* c, const lfgpu_transcript_ops* ts) {
    if (!ts->write_elt_sized || !ts->write_elt_array_sized)
      return lf_fail(c, LFGPU_ERR_ARG, "zk256: the transcript hooks lack write_elt_sized / write_elt_array_sized (32-byte elements)");
    return LFGPU_OK;
  }
  // a hand-made lfgpu_ligero_param: the flat positions of a_terms256_kernel
  static bool ligero_param_ok(const lfgpu_ligero_param& p) { return p.nw <= p.nwrow * p.w && p.nq <= p.nqtriples * p.w && p.nwqrow * p.w < 0xffffffffull; }
  static int eq_store(lfgpu_ctx*, size_t, void* own, E** d_eq) {  // the prover's own table, or the batch's first
    *d_eq = (E*)own;
    return LFGPU_OK;
  }
  static int batch_prepare(lfgpu_ctx* c, size_t) { return scb256_mailbox(c); }  // the context's pinned mailbox of the batched sumcheck
  static int lig_commit(lfgpu_ctx* c, const lfgpu_circuit_info&, const lfgpu_ligero_param& p, const E* W, const size_t* lqc, lfgpu_rng_fn rng, void* user,
                        uint8_t root[32], Lig** out, const lfgpu_comm_ops* shard) {
    return lig256_commit(c, p, W, lqc, rng, user, root, out, shard);
  }
  static int lig_commit_batch(lfgpu_ctx* c, const lfgpu_circuit_info&, const lfgpu_ligero_param& p, size_t nb, const E* const* W, const size_t* lqc,
                              const lfgpu_rng_fn* rng, void* const* users, uint8_t* roots, Lig** out) {
    return lig256_commit_batch(c, p, nb, W, lqc, rng, users, roots, out);
  }
  static void lig_free(Lig* lp) { delete lp; }  // ~Slab scrubs the buffers and returns them to the context's pool
  // the Ligero layout's draws on the empty slab: no image, the nonces dropped
  static int draws_only(lfgpu_ctx* c, const lfgpu_ligero_param& p, const E* W, const size_t* lqc, lfgpu_rng_fn rng, void* user) {
    char err[256] = {0};
    const int rc = lig::layout(L32(), p, W, 0, lqc, rng, user, c->rng_exact != 0, 0, 0, (E*)nullptr, nullptr, err);
    return rc ? lf_fail(c, rc, "%s", err) : LFGPU_OK;
  }
};
}  // namespace

// ------------------------------------------------------------------ ZkProver<Fp256Base>
// P32, L32 and the kernels stay in this file (zkint.h), so the cross-file functions below are where the driver layer of
// zk_driver.h is instantiated for the policy: the records are zkp::Prover<P32> / zkp::Batch<P32>, every function one call.
struct Zk256 : zkp::Prover<P32> {};
struct Zk256Batch : zkp::Batch<P32> {};

int zk256_new(lfgpu_ctx* c, const lfgpu_circuit* C, size_t rateinv, size_t nreq, size_t block_enc, Zk256** out) {
  std::unique_ptr<Zk256> z(new Zk256());
  LF_TRY(zkp::prover_init<P32>(*z, c, C, rateinv, nreq, block_enc));
  *out = z.release();
  return LFGPU_OK;
}
int zk256_param(const Zk256* z, lfgpu_ligero_param* p) {
  *p = z->st.param;
  return LFGPU_OK;
}
void zk256_set_comm(Zk256* z, const lfgpu_comm_ops* comm, size_t min_tableau_bytes) {
  z->have_comm = comm != nullptr;
  if (comm) z->comm = *comm;
  z->comm_min_bytes = min_tableau_bytes;
}
const lfgpu_comm_ops* zk256_comm(const Zk256* z) { return z->have_comm ? &z->comm : nullptr; }
void zk256_free(Zk256* z) { delete z; }
int zk256_timings(const Zk256* z, double ms[6]) {
  memcpy(ms, z->st.ms, sizeof(z->st.ms));
  return LFGPU_OK;
}
int zk256_commit(Zk256* z, const void* h_W, lfgpu_rng_fn rng, void* rng_user, const lfgpu_transcript_ops* ts, uint8_t root_out[32], bool draws_only) {
  return zkp::commit<P32>(*z, h_W, rng, rng_user, ts, root_out, draws_only);
}
int zk256_prove(Zk256* z, const void* h_W, const lfgpu_transcript_ops* tso, int* ok) { return zkp::prove<P32>(*z, h_W, tso, ok); }
int zk256_proof_write(const Zk256* z, uint8_t* buf, size_t cap, size_t* nbytes) { return zkp::proof_write_cached(z->c, P32(), z->C, z->st, buf, cap, nbytes); }

int zk256_batch_new(lfgpu_ctx* c, const lfgpu_circuit* C, size_t nb_max, Zk256Batch** out) {
  std::unique_ptr<Zk256Batch> bt(new Zk256Batch());
  LF_TRY(zkp::batch_init<P32>(*bt, c, C, nb_max));
  *out = bt.release();
  return LFGPU_OK;
}
void zk256_batch_free(Zk256Batch* bt) { delete bt; }
int zk256_prove_batch(Zk256Batch* bt, Zk256* const* z, size_t nb, const void* const* h_W, const lfgpu_transcript_ops* const* ts, int* ok) {
  return zkp::prove_batch<P32>(*bt, z, nb, h_W, ts, ok);
}
int zk256_commit_batch(Zk256Batch* bt, Zk256* const* z, size_t nb, const void* const* h_W, const lfgpu_rng_fn* rng, void* const* rng_user,
                       const lfgpu_transcript_ops* const* ts, uint8_t* roots_out) {
  return zkp::commit_batch<P32>(*bt, z, nb, h_W, rng, rng_user, ts, roots_out);
}

int zk256_verify(lfgpu_ctx* c, const lfgpu_circuit* C, size_t rateinv, size_t nreq, size_t block_enc, const uint8_t* proof, size_t proof_len, const void* h_pub,
                 const lfgpu_transcript_ops* tso, bool committed, int* ok, const char** why_out) {
  *ok = 0;
  LF_TRY(P32::ts_ok(c, tso));
  const lfgpu_circuit_info& I = C->info;
  lfgpu_ligero_param p{};
  LF_TRY(lfgpu_ligero_param_init(&p, LFGPU_FIELD_P256, 0, I.ninputs - I.npub_in + zkp::pad_size(C), C->layers.size(), rateinv, nreq, block_enc));
  auto eq_table = [&](E** d_eq) {  // the head of the verifier's device buffer (P32::verifier_ext)
    void* dv = nullptr;
    LF_TRY(lf_scratch4(c, P32::verifier_bytes(I, p), &dv));
    *d_eq = (E*)dv;
    return (int)LFGPU_OK;
  };
  return zkp::verify<P32>(c, C, P32(), p, proof, proof_len, h_pub, tso, committed, eq_table, ok, why_out);
}

// ------------------------------------------------------------------ LigeroProver::prove / LigeroVerifier::verify on a caller's statement
// zkp::ligero_prove_entry / ligero_verify_entry (zk_driver.h) over Fp256Base: the sized hooks checked in front (the parameter
// checks of the kernel's flat positions: P32::ligero_param_ok), the A step is L32::a_rows_terms on the caller's term list.
extern "C" int lfgpu_ligero_prove256(lfgpu_ligero_prover* lp, const lfgpu_transcript_ops* tso, size_t nl, size_t nllterm, const lfgpu_ligero_llterm256* llterm,
                                     const uint8_t hash_of_llterm[32], const size_t* h_lqc, uint8_t* buf, size_t cap, size_t* nbytes) {
  auto pre = [&](const LfLigeroView& v, Lig32** lig) {
    if (!v.lig256) return lf_fail(v.c, LFGPU_ERR_ARG, "ligero_prove256: the prover is not over Fp256Base (lfgpu_ligero_prove serves the 16-byte fields)");
    *lig = lig32_of(v.lig256);
    return P32::ts_ok(v.c, tso);
  };
  auto dot = [&](Lig32* L, const std::vector<E>& alphal, const std::vector<E>& alphaq, E* y_dot) {
    const Terms256 t{llterm, nllterm, alphal.data(), nl, h_lqc, alphaq.data()};
    return lig::dot_terms(L, L32(), t, y_dot);
  };
  return zkp::ligero_prove_entry<P32>("ligero_prove256", lp, tso, nl, nllterm, llterm, hash_of_llterm, h_lqc, buf, cap, nbytes, pre, dot);
}

extern "C" int lfgpu_ligero_verify256(lfgpu_ctx* c, const lfgpu_ligero_param* pp, const uint8_t root[32], const uint8_t* proof, size_t proof_len,
                                      const lfgpu_transcript_ops* tso, size_t nl, size_t nllterm, const lfgpu_ligero_llterm256* llterm,
                                      const uint8_t hash_of_llterm[32], const void* h_b, const size_t* h_lqc, int* ok, const char** why_out) {
  auto pre = [&] { return P32::ts_ok(c, tso); };
  auto ext = [&](const zkp::ComProof<E>& pr, const std::vector<E>& alphal, const std::vector<E>& alphaq, const size_t* idx, std::vector<E>& out) {
    const lfgpu_ligero_param& p = *pp;
    const Terms256 t{llterm, nllterm, alphal.data(), nl, h_lqc, alphaq.data()};
    auto a_rows = [&](E* d_T, size_t ld) { return L32::a_rows_terms(c, p, ld, t, d_T); };
    void* dv = nullptr;
    LF_TRY(lf_scratch4(c, (p.nwqrow + 3) * (p.block_enc + p.nreq) * 32 + 256, &dv));
    return P32::verifier_ext_with(c, p, (E*)dv, a_rows, pr, idx, out);
  };
  return zkp::ligero_verify_entry<P32>("ligero_verify256", c, LFGPU_FIELD_P256, 0, pp, root, proof, proof_len, tso, nl, nllterm, llterm, hash_of_llterm, h_b, h_lqc,
                                       ok, why_out, pre, ext);
}
