// p256.hip -- the P-256 base-field leg of the path (field id 1, 32-byte elements): BASELINE config 5's signature
// tableau, ZkProver<Fp256Base, ReedSolomonFactory<Fp256Base, FFTExtConvolutionFactory>> (reference
// lib/circuits/mdoc/mdoc_zk.cc:70-88,485-500).
//
//   K4' lfgpu_fp256_rs_encode_rows : ReedSolomon<Fp256Base, FFTExtConvolution>::interpolate over the rows of a tableau
//        (lib/algebra/reed_solomon.h:51-110, convolution.h:129-191, rfft.h:282-376)
//   K5' column_leaves32_kernel     : LigeroCommon<Fp256Base>::column_hash (lib/ligero/ligero_param.h:432-439)
//   field binops                   : FpGeneric::addf / subf / mulf for the parity tests
//
// The reference computes the convolution with a REAL fft in half-complex storage (RFFT over Fp2, because Fp256 itself
// has no 2^k-th roots of unity: p - 1 = 2 * odd).  The convolution is a well-defined element of the field, so any exact
// method returns the same 32 bytes; the device uses what maps to a GPU: two tableau rows a, b travel as ONE complex
// sequence a + i b through a radix-2 FFT over Fp2 = Fp256[i] (decimation in frequency forward, decimation in time
// backward, so no bit-reversal pass), the kernel y (1/k) is real, hence conv(a + i b, y) = conv(a, y) + i conv(b, y).
// Twiddles: powers of the reference's root of order 2^31 on the unit circle (mdoc_zk.cc:82-88): w^-1 = conj(w).
#include <string>

#include "ctx.h"
#include "fp256.h"

#define P256_LOCAL_LOG 9  // points per LDS tile of the local FFT kernel: 512 x 64 B = 32 KiB

LF_HD fp2_t fp2_conj(const fp2_t& a) { return fp2_t{a.re, fp256_neg(a.im)}; }
__device__ inline fp2_t ldc(const fp2_t* p) { return fp2_t{ld32(&p->re), ld32(&p->im)}; }
__device__ inline void stc(fp2_t* p, const fp2_t& v) {
  st32(&p->re, v.re);
  st32(&p->im, v.im);
}

// ------------------------------------------------------------------ FFT over Fp2
// one radix-2 stage on global memory, half-distance h; W[j] = w_P^j (j < P/2)
//   forward (DIF): (u, v) -> (u + v, (u - v) conj(W[k P/2h]))      backward (DIT): (u, v W[k P/2h]) -> (u + v, u - v)
template <bool FWD>
__global__ void fp2_fft_stage_kernel(fp2_t* __restrict__ Z, u32 P, u32 h, const fp2_t* __restrict__ W) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P / 2) return;
  const u32 k = t & (h - 1), i = ((t - k) << 1) | k;
  fp2_t* z = Z + (size_t)blockIdx.y * P;
  const fp2_t w = ldc(&W[(size_t)k * (P / (2 * h))]);
  fp2_t u = ldc(&z[i]), v = ldc(&z[i + h]);
  if (FWD) {
    stc(&z[i], fp2_add(u, v));
    stc(&z[i + h], fp2_mul(fp2_sub(u, v), fp2_conj(w)));
  } else {
    v = fp2_mul(v, w);
    stc(&z[i], fp2_add(u, v));
    stc(&z[i + h], fp2_sub(u, v));
  }
}
// the stages with half-distance < 2^tl on a contiguous tile of 2^tl points in LDS (forward: the last tl stages,
// backward: the first tl)
template <bool FWD>
__global__ __launch_bounds__(256) void fp2_fft_local_kernel(fp2_t* __restrict__ Z, u32 P, u32 tl, const fp2_t* __restrict__ W) {
  extern __shared__ uint4 lds4[];
  fp2_t* s = reinterpret_cast<fp2_t*>(lds4);
  const u32 L = 1u << tl, tid = threadIdx.x;
  fp2_t* z = Z + (size_t)blockIdx.y * P + (size_t)blockIdx.x * L;
  for (u32 i = tid; i < L; i += 256) s[i] = ldc(&z[i]);
  __syncthreads();
  for (u32 st = 0; st < tl; ++st) {
    const u32 h = FWD ? (L >> (st + 1)) : (1u << st);
    for (u32 t = tid; t < L / 2; t += 256) {
      const u32 k = t & (h - 1), i = ((t - k) << 1) | k;
      const fp2_t w = ldc(&W[(size_t)k * (P / (2 * h))]);
      fp2_t u = s[i], v = s[i + h];
      if (FWD) {
        s[i] = fp2_add(u, v);
        s[i + h] = fp2_mul(fp2_sub(u, v), fp2_conj(w));
      } else {
        v = fp2_mul(v, w);
        s[i] = fp2_add(u, v);
        s[i + h] = fp2_sub(u, v);
      }
    }
    __syncthreads();
  }
  for (u32 i = tid; i < L; i += 256) stc(&z[i], s[i]);
}

static int fp2_fft(lfgpu_ctx* c, bool fwd, size_t batch, u32 P, fp2_t* Z, const fp2_t* W) {
  if (P < 2 || batch == 0) return LFGPU_OK;
  const u32 lp = lf_log2(P), tl = lp < P256_LOCAL_LOG ? lp : P256_LOCAL_LOG;
  const dim3 gs((P / 2 + 255) / 256, (u32)batch), gl(P >> tl, (u32)batch);
  const size_t lds = (size_t)64 << tl;
  if (fwd) {
    for (u32 h = P / 2; h >= (1u << tl); h >>= 1) hipLaunchKernelGGL(fp2_fft_stage_kernel<true>, gs, dim3(256), 0, c->stream, Z, P, h, W);
    hipLaunchKernelGGL(fp2_fft_local_kernel<true>, gl, dim3(256), lds, c->stream, Z, P, tl, W);
  } else {
    hipLaunchKernelGGL(fp2_fft_local_kernel<false>, gl, dim3(256), lds, c->stream, Z, P, tl, W);
    for (u32 h = 1u << tl; h <= P / 2; h <<= 1) hipLaunchKernelGGL(fp2_fft_stage_kernel<false>, gs, dim3(256), 0, c->stream, Z, P, h, W);
  }
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}

// ------------------------------------------------------------------ Reed-Solomon rows
// One complex row of the convolution's input: z[i] = binom[i] * (row0[i] + i row1[i]) for i < n, 0 up to P (reed_solomon.h:101-104);
// row1 == nullptr: the odd last row, its imaginary part stays zero.  The body of p256_rs_pre_kernel and of its batched twin.
__device__ __forceinline__ void p256_rs_pre_row(u32 i, u32 n, const elt32_t* __restrict__ binom, const elt32_t* __restrict__ row0,
                                                const elt32_t* __restrict__ row1, fp2_t* __restrict__ z) {
  fp2_t v{e32_zero(), e32_zero()};
  if (i < n) {
    const elt32_t b = ld32(&binom[i]);
    v.re = fp256_mul(b, ld32(&row0[i]));
    if (row1) v.im = fp256_mul(b, ld32(&row1[i]));
  }
  stc(&z[i], v);
}
// ... and of its output: row[k] = lead[k - (n-1)] * conv[k] for n <= k < m (reed_solomon.h:106-109); row1 == nullptr: nothing is
// written for the imaginary part
__device__ __forceinline__ void p256_rs_post_row(u32 i, u32 n, const elt32_t* __restrict__ lead, const fp2_t* __restrict__ z,
                                                 elt32_t* __restrict__ row0, elt32_t* __restrict__ row1) {
  const elt32_t l = ld32(&lead[i - (n - 1)]);
  const fp2_t v = ldc(&z[i]);
  st32(&row0[i], fp256_mul(l, v.re));
  if (row1) st32(&row1[i], fp256_mul(l, v.im));
}
// Z[pair] from rows 2 pair, 2 pair + 1 of one tableau
__global__ void p256_rs_pre_kernel(u32 n, u32 P, u32 nrow, const elt32_t* __restrict__ binom, const elt32_t* __restrict__ T, size_t ld,
                                   fp2_t* __restrict__ Z) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const u32 r0 = 2 * blockIdx.y, r1 = r0 + 1;
  p256_rs_pre_row(i, n, binom, T + (size_t)r0 * ld, r1 < nrow ? T + (size_t)r1 * ld : nullptr, Z + (size_t)blockIdx.y * P);
}
// Z[k] *= yhat[k] (both in the forward transform's bit-reversed order)
__global__ void p256_rs_pointwise_kernel(u32 P, const fp2_t* __restrict__ yhat, fp2_t* __restrict__ Z) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  fp2_t* z = &Z[(size_t)blockIdx.y * P + i];
  stc(z, fp2_mul(ldc(z), ldc(&yhat[i])));
}
// rows 2 pair, 2 pair + 1 of one tableau from Z[pair]
__global__ void p256_rs_post_kernel(u32 n, u32 m, u32 P, u32 nrow, const elt32_t* __restrict__ lead, const fp2_t* __restrict__ Z,
                                    elt32_t* __restrict__ T, size_t ld) {
  const u32 i = n + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const u32 r0 = 2 * blockIdx.y, r1 = r0 + 1;
  p256_rs_post_row(i, n, lead, Z + (size_t)blockIdx.y * P, T + (size_t)r0 * ld, r1 < nrow ? T + (size_t)r1 * ld : nullptr);
}

// The batched twins: one row group of cb tableaux of one shape through ONE convolution.  The group's rows are numbered through all
// statements, q = b * gr + r (statement b, r-th row of the group), and rows 2 pair, 2 pair + 1 of that numbering share a complex
// transform -- across statements too, so a one-row group does not leave every imaginary half empty (the arithmetic is exact:
// the pairing does not change a value).  Row r of the group is tableau row base + r, or base + r + skip from r = seg on (the
// group [0, idot) + [iquad + 1, nrow) is base 0, seg idot, skip 2).  Statement and row follow from blockIdx.y alone: the base
// pointers are scalar loads from the kernarg segment.
struct P256RowGroup {
  u32 total, gr, base, seg, skip;  // total = cb * gr rows
};
__device__ __forceinline__ elt32_t* p256_group_row(const LfBatchPtrs& T, size_t ld, const P256RowGroup& g, u32 q) {
  const u32 b = q / g.gr, r = q - b * g.gr;
  return (elt32_t*)T.p[b] + (size_t)(g.base + r + (r >= g.seg ? g.skip : 0u)) * ld;
}
__global__ void p256_rs_pre_batch_kernel(u32 n, u32 P, P256RowGroup g, const elt32_t* __restrict__ binom, LfBatchPtrs T, size_t ld, fp2_t* __restrict__ Z) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const u32 q0 = 2 * blockIdx.y, q1 = q0 + 1;
  p256_rs_pre_row(i, n, binom, p256_group_row(T, ld, g, q0), q1 < g.total ? p256_group_row(T, ld, g, q1) : nullptr, Z + (size_t)blockIdx.y * P);
}
__global__ void p256_rs_post_batch_kernel(u32 n, u32 m, u32 P, P256RowGroup g, const elt32_t* __restrict__ lead, const fp2_t* __restrict__ Z, LfBatchPtrs T,
                                          size_t ld) {
  const u32 i = n + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const u32 q0 = 2 * blockIdx.y, q1 = q0 + 1;
  p256_rs_post_row(i, n, lead, Z + (size_t)blockIdx.y * P, p256_group_row(T, ld, g, q0), q1 < g.total ? p256_group_row(T, ld, g, q1) : nullptr);
}

// host-side field helpers: fp256.h
static elt32_t h256_dec(const char* s) {
  elt32_t r = e32_zero();
  const elt32_t ten = h256_of_scalar(10);
  for (; *s; ++s) r = fp256_add(fp256_mul(r, ten), h256_of_scalar((u64)(*s - '0')));
  return r;
}

// W[j] = w_P^j, j < P/2, w_P = the reference's root of order 2^31 re-rooted (lib/algebra/twiddle.h:36-55)
static int p256_twiddles(lfgpu_ctx* c, u32 P, const fp2_t** out) {
  char kb[48];
  snprintf(kb, sizeof(kb), "p256tw:%u", P);
  void* d = nullptr;
  if (!lf_table_lookup(c, kb, &d)) {
    fp2_t w{h256_dec("112649224146410281873500457609690258373018840430489408729223714171582664680802"),
            h256_dec("84087994358540907695740461427818660560182168997182378749313018254450460212908")};
    for (u64 r = P; r < ((u64)1 << 31); r += r) w = fp2_mul(w, w);
    std::vector<fp2_t> t(P / 2 ? P / 2 : 1);
    fp2_t x{h256_of_scalar(1), e32_zero()};
    for (u32 i = 0; 2 * i < P; ++i) {
      t[i] = x;
      x = fp2_mul(x, w);
    }
    LF_TRY(lf_table(c, kb, t.data(), t.size() * sizeof(fp2_t), &d));
  }
  *out = (const fp2_t*)d;
  return LFGPU_OK;
}

// The device tables of the extension n -> m (0 < n < m): the twiddles of its transform size P and the constants of the ReedSolomon
// ctor.  Built on first use, with synchronous copies and a stream synchronise; a later call only looks them up.
struct P256RsTables {
  size_t P;
  const fp2_t *W, *yhat;
  const elt32_t *binom, *lead;
};
static int p256_rs_tables(lfgpu_ctx* c, const char* who, size_t n, size_t m, P256RsTables* out) {
  size_t P = 1;
  while (P < m) P <<= 1;
  if (P > ((size_t)1 << 24)) return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "%s: m > 2^24", who);
  const fp2_t* W = nullptr;
  LF_TRY(p256_twiddles(c, (u32)P, &W));
  const size_t d = n - 1;
  char kb[96];
  snprintf(kb, sizeof(kb), "p256rs:%zu:%zu", n, m);
  const std::string key(kb);
  void *dbinom = nullptr, *dlead = nullptr, *dyhat = nullptr;
  if (!lf_table_lookup(c, key + ":yhat", &dyhat)) {
    // constants of the ReedSolomon ctor (reed_solomon.h:51-88), batch inverse as AlgebraUtil::batch_inverse_arithmetic
    std::vector<elt32_t> inv(m), lead(m - n + 1), binom(n);
    const elt32_t one = h256_of_scalar(1), zero = e32_zero();
    {
      std::vector<elt32_t> pre(m);
      elt32_t acc = one;
      for (size_t i = 1; i < m; ++i) {
        pre[i] = acc;
        acc = fp256_mul(acc, h256_of_scalar(i));
      }
      elt32_t ia = m > 1 ? h256_inv(acc) : acc;
      inv[0] = zero;
      for (size_t i = m; i-- > 1;) {
        inv[i] = fp256_mul(ia, pre[i]);
        ia = fp256_mul(ia, h256_of_scalar(i));
      }
    }
    lead[0] = one;
    binom[0] = one;
    for (size_t i = 1; i + d < m; ++i) lead[i] = fp256_mul(lead[i - 1], fp256_mul(h256_of_scalar(d + i), inv[i]));
    for (size_t kk = d; kk < m; ++kk) {
      lead[kk - d] = fp256_mul(lead[kk - d], h256_of_scalar(kk - d));
      if (d % 2 == 1) lead[kk - d] = fp256_neg(lead[kk - d]);
    }
    for (size_t i = 1; i < n; ++i) binom[i] = fp256_mul(binom[i - 1], fp256_mul(h256_of_scalar(n - i), inv[i]));
    for (size_t i = 1; i < n; i += 2) binom[i] = fp256_neg(binom[i]);
    // yhat = forward transform of the padded inverses, divided by P (convolution.h:136-152), in bit-reversed order
    std::vector<fp2_t> yh(P, fp2_t{zero, zero});
    for (size_t i = 0; i < m; ++i) yh[i].re = inv[i];
    void* tmp = nullptr;
    LF_TRY(lf_scratch2(c, P * sizeof(fp2_t), &tmp));
    LF_HIP(c, hipMemcpy(tmp, yh.data(), P * sizeof(fp2_t), hipMemcpyHostToDevice));
    LF_TRY(fp2_fft(c, true, 1, (u32)P, (fp2_t*)tmp, W));
    LF_HIP(c, hipStreamSynchronize(c->stream));
    LF_HIP(c, hipMemcpy(yh.data(), tmp, P * sizeof(fp2_t), hipMemcpyDeviceToHost));
    const elt32_t sc = h256_inv(h256_of_scalar(P));
    for (size_t i = 0; i < P; ++i) yh[i] = fp2_t{fp256_mul(yh[i].re, sc), fp256_mul(yh[i].im, sc)};
    LF_TRY(lf_table(c, key + ":binom", binom.data(), binom.size() * 32, &dbinom));
    LF_TRY(lf_table(c, key + ":lead", lead.data(), lead.size() * 32, &dlead));
    LF_TRY(lf_table(c, key + ":yhat", yh.data(), yh.size() * sizeof(fp2_t), &dyhat));
  } else {
    lf_table_lookup(c, key + ":binom", &dbinom);
    lf_table_lookup(c, key + ":lead", &dlead);
  }
  *out = P256RsTables{P, W, (const fp2_t*)dyhat, (const elt32_t*)dbinom, (const elt32_t*)dlead};
  return LFGPU_OK;
}

extern "C" int lfgpu_fp256_rs_encode_rows(lfgpu_ctx* c, size_t nrow, size_t n, size_t m, void* d_T, size_t ld) {
  if (!c || (!d_T && nrow)) return lf_fail(c, LFGPU_ERR_ARG, "fp256_rs_encode_rows: null argument");
  if (n == 0 || m < n || ld < m) return lf_fail(c, LFGPU_ERR_ARG, "fp256_rs_encode_rows: need 0 < n <= m <= ld");
  if (nrow == 0 || m == n) return LFGPU_OK;
  LF_HIP(c, hipSetDevice(c->device));
  P256RsTables t;
  LF_TRY(p256_rs_tables(c, "fp256_rs_encode_rows", n, m, &t));
  const size_t P = t.P, npair = (nrow + 1) / 2;
  void* Zv = nullptr;
  LF_TRY(lf_scratch2(c, npair * P * sizeof(fp2_t), &Zv));
  fp2_t* Z = (fp2_t*)Zv;
  const dim3 gp((u32)((P + 255) / 256), (u32)npair);
  hipLaunchKernelGGL(p256_rs_pre_kernel, gp, dim3(256), 0, c->stream, (u32)n, (u32)P, (u32)nrow, t.binom, (const elt32_t*)d_T, ld, Z);
  LF_TRY(fp2_fft(c, true, npair, (u32)P, Z, t.W));
  hipLaunchKernelGGL(p256_rs_pointwise_kernel, gp, dim3(256), 0, c->stream, (u32)P, t.yhat, Z);
  LF_TRY(fp2_fft(c, false, npair, (u32)P, Z, t.W));
  const dim3 go((u32)((m - n + 255) / 256), (u32)npair);
  hipLaunchKernelGGL(p256_rs_post_kernel, go, dim3(256), 0, c->stream, (u32)n, (u32)m, (u32)P, (u32)nrow, t.lead, (const fp2_t*)Z, (elt32_t*)d_T, ld);
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}

// ---- the batched commit's encoder (zk256.hip: lig256_commit_batch)
// The tables of the extension n -> m exist when this returns: called for every shape of a chain before anything is enqueued, so
// that the chain itself never meets the first-use set-up (synchronous copies and a synchronise)
int lf_p256_rs_prepare(lfgpu_ctx* c, size_t n, size_t m) {
  if (n == 0 || m < n) return lf_fail(c, LFGPU_ERR_ARG, "p256_rs_prepare: need 0 < n <= m");
  if (m == n) return LFGPU_OK;
  P256RsTables t;
  return p256_rs_tables(c, "p256_rs_prepare", n, m, &t);
}
// convolution scratch of `rows` rows of an extension to m, in bytes; 0: more row pairs than one launch's gridDim.y holds
size_t lf_p256_rs_batch_scratch(size_t rows, size_t m) {
  size_t P = 1;
  while (P < m) P <<= 1;
  const size_t pairs = (rows + 1) / 2;
  return pairs <= 65535 ? pairs * P * sizeof(fp2_t) : 0;
}
// One row group of cb tableaux (statement b at T.p[b], stride ld), gr rows each, n values long, extended to m in place through
// ONE convolution of cb * gr rows: group row r is tableau row base + r, from r = seg on base + r + skip.  Z: the convolution
// scratch, lf_p256_rs_batch_scratch(cb * gr, m) bytes.  Enqueue only.
int lf_p256_rs_rows_batch(lfgpu_ctx* c, size_t cb, const LfBatchPtrs& T, size_t base, size_t seg, size_t skip, size_t gr, size_t n, size_t m, size_t ld,
                          void* d_Z) {
  if (cb == 0 || gr == 0 || m == n) return LFGPU_OK;
  const size_t total = cb * gr, npair = (total + 1) / 2;
  if (cb > LFGPU_SC_BATCH_MAX || npair > 65535 || n == 0 || m < n || ld < m || !d_Z) return lf_fail(c, LFGPU_ERR_ARG, "p256_rs_rows_batch: bad argument");
  P256RsTables t;
  LF_TRY(p256_rs_tables(c, "p256_rs_rows_batch", n, m, &t));  // (a lookup: lf_p256_rs_prepare has run)
  const u32 P = (u32)t.P;
  fp2_t* Z = (fp2_t*)d_Z;
  const P256RowGroup g{(u32)total, (u32)gr, (u32)base, (u32)seg, (u32)skip};
  const dim3 gp((P + 255) / 256, (u32)npair);
  hipLaunchKernelGGL(p256_rs_pre_batch_kernel, gp, dim3(256), 0, c->stream, (u32)n, P, g, t.binom, T, ld, Z);
  LF_TRY(fp2_fft(c, true, npair, P, Z, t.W));
  hipLaunchKernelGGL(p256_rs_pointwise_kernel, gp, dim3(256), 0, c->stream, P, t.yhat, Z);
  LF_TRY(fp2_fft(c, false, npair, P, Z, t.W));
  const dim3 go((u32)((m - n + 255) / 256), (u32)npair);
  hipLaunchKernelGGL(p256_rs_post_batch_kernel, go, dim3(256), 0, c->stream, (u32)n, (u32)m, P, g, t.lead, (const fp2_t*)Z, T, ld);
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}

// Host-buffer form (what GpuReedSolomon<Fp256Base>::interpolate calls from inside the reference's LigeroProver): stage in
// scratch4 -- the encode itself works through scratch2.
extern "C" int lfgpu_fp256_rs_encode_rows_host(lfgpu_ctx* c, size_t nrow, size_t n, size_t m, void* h_T, size_t ld) {
  if (!c || (!h_T && nrow)) return lf_fail(c, LFGPU_ERR_ARG, "fp256_rs_encode_rows_host: null argument");
  if (n == 0 || m < n || ld < m) return lf_fail(c, LFGPU_ERR_ARG, "fp256_rs_encode_rows_host: need 0 < n <= m <= ld");
  if (nrow == 0 || m == n) return LFGPU_OK;
  LF_HIP(c, hipSetDevice(c->device));
  void* d = nullptr;
  const size_t bytes = ((nrow - 1) * ld + m) * sizeof(elt32_t);
  LF_TRY(lf_scratch4(c, bytes, &d));
  LF_HIP(c, hipMemcpyAsync(d, h_T, bytes, hipMemcpyHostToDevice, c->stream));
  LF_TRY(lfgpu_fp256_rs_encode_rows(c, nrow, n, m, d, ld));
  LF_HIP(c, hipMemcpyAsync(h_T, d, bytes, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipStreamSynchronize(c->stream));
  return LFGPU_OK;
}

// ------------------------------------------------------------------ column hash, 32-byte elements
// leaf_j = SHA256(nonce_j[32] || canon(T[0][col0+j]) || ... ), canon = 32 little-endian bytes of the value out of
// Montgomery form.  One lane per column; a row read is two coalesced 16 B/lane loads per lane.
// (the body of column_leaves32_kernel and of its batched twin: col = the column's first element, nonce = its 32 bytes, out = its leaf)
__device__ __forceinline__ void column_leaf32(u32 nrow, size_t ld, const elt32_t* __restrict__ col, const uint4* __restrict__ nonce, uint4* __restrict__ out) {
  sha_state st;
  sha_init(st);
  const u32 nch = 2 + 2 * nrow;                  // 16-byte chunks of message
  const u32 nblk = (nch * 16 + 9 + 63) / 64;
  const u64 bits = (u64)nch * 128;
  elt32_t cur = e32_zero();
  for (u32 bi = 0; bi < nblk; ++bi) {
    u32 w[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u32 ch = 4 * bi + q;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (ch < 2) {
        const uint4 nb = nonce[ch];
        v = make_uint4(bswap32(nb.x), bswap32(nb.y), bswap32(nb.z), bswap32(nb.w));
      } else if (ch < nch) {
        const u32 e = ch - 2;
        if ((e & 1) == 0) cur = fp256_canon(ld32(col + (size_t)(e >> 1) * ld));
        const u64 lo = cur.l[2 * (e & 1)], hi = cur.l[2 * (e & 1) + 1];
        v = make_uint4(bswap32((u32)lo), bswap32((u32)(lo >> 32)), bswap32((u32)hi), bswap32((u32)(hi >> 32)));
      } else if (ch == nch) {
        v.x = 0x80000000u;
      }
      w[4 * q + 0] = v.x;
      w[4 * q + 1] = v.y;
      w[4 * q + 2] = v.z;
      w[4 * q + 3] = v.w;
    }
    if (bi == nblk - 1) {
      w[14] = (u32)(bits >> 32);
      w[15] = (u32)bits;
    }
    sha_compress(st, w);
  }
  out[0] = make_uint4(bswap32(st.h[0]), bswap32(st.h[1]), bswap32(st.h[2]), bswap32(st.h[3]));
  out[1] = make_uint4(bswap32(st.h[4]), bswap32(st.h[5]), bswap32(st.h[6]), bswap32(st.h[7]));
}
__global__ __launch_bounds__(256) void column_leaves32_kernel(u32 nrow, size_t ld, size_t col0, u32 ncols, const elt32_t* __restrict__ T,
                                                              const uint4* __restrict__ nonces, uint4* __restrict__ out, size_t out0) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ncols) return;
  column_leaf32(nrow, ld, T + col0 + j, nonces + 2 * (size_t)j, out + 2 * (out0 + j));
}
// nb tableaux of one shape: statement blockIdx.y hashes its columns with nonces [b][ncols][32] into leaf level ncols of its own heap
__global__ __launch_bounds__(256) void column_leaves32_batch_kernel(u32 nrow, size_t ld, size_t col0, u32 ncols, LfBatchPtrs T, const uint4* __restrict__ nonces,
                                                                    LfBatchPtrs layers) {
  const u32 b = blockIdx.y;
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ncols) return;
  column_leaf32(nrow, ld, (const elt32_t*)T.p[b] + col0 + j, nonces + 2 * ((size_t)b * ncols + j), (uint4*)layers.p[b] + 2 * ((size_t)ncols + j));
}
int lf_column_leaves32(lfgpu_ctx* c, size_t nrow, size_t ld, size_t col0, size_t ncols, const void* d_T, const void* d_nonces, void* d_out,
                       size_t out0) {
  hipLaunchKernelGGL(column_leaves32_kernel, dim3((u32)((ncols + 255) / 256)), dim3(256), 0, c->stream, (u32)nrow, ld, col0, (u32)ncols,
                     (const elt32_t*)d_T, (const uint4*)d_nonces, (uint4*)d_out, out0);
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}
// enqueue only; the caller has checked the shape (lfgpu_column_commit_batch256)
int lf_column_leaves32_batch(lfgpu_ctx* c, size_t nrow, size_t ld, size_t col0, size_t ncols, size_t nb, const LfBatchPtrs& T, const void* d_nonces,
                             const LfBatchPtrs& layers) {
  hipLaunchKernelGGL(column_leaves32_batch_kernel, dim3((u32)((ncols + 255) / 256), (u32)nb), dim3(256), 0, c->stream, (u32)nrow, ld, col0, (u32)ncols, T,
                     (const uint4*)d_nonces, layers);
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}

// ------------------------------------------------------------------ element-wise ops
__global__ void p256_binop_kernel(int op, size_t n, const elt32_t* __restrict__ a, const elt32_t* __restrict__ b, elt32_t* __restrict__ o) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const elt32_t x = ld32(&a[i]), y = ld32(&b[i]);
  st32(&o[i], op == 0 ? fp256_add(x, y) : op == 1 ? fp256_sub(x, y) : fp256_mul(x, y));
}
int lf_p256_binop(lfgpu_ctx* c, int op, size_t n, const void* d_a, const void* d_b, void* d_out) {
  hipLaunchKernelGGL(p256_binop_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, c->stream, op, n, (const elt32_t*)d_a, (const elt32_t*)d_b,
                     (elt32_t*)d_out);
  LF_HIP(c, hipGetLastError());
  return LFGPU_OK;
}
