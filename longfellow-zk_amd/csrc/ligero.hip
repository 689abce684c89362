// ligero.hip -- LigeroProver::commit / prove on a device-resident tableau.
//
// Reference: LigeroParam::layout (lib/ligero/ligero_param.h:185-295),
// LigeroProver::commit / layout_* / low_degree_proof / dot_proof / quadratic_proof /
// compute_req (lib/ligero/ligero_prover.h:58-79,171-351), MerkleCommitment
// (lib/merkle/merkle_commitment.h:50-73).
//
// Host side: all RandomEngine draws happen on the host in the reference's order (they do
// not depend on computed data), the un-encoded rows are assembled in one host buffer and
// uploaded once; the GPU then RS-encodes every row (K3/K4) and commits the columns
// (K5/K6).  The tableau stays in HBM for the prove-side row combinations (K12).
#include <algorithm>
#include <memory>
#include <new>

#include "ctx.h"
#include "ligero_slab.h"
#include "runfold.h"
#include "zkint.h"

// the C ABI's opaque prover: the shared record (ligero_slab.h) over 16-byte elements, plus which field it serves.  For field
// P256 the record over 32-byte elements lives in zk256.hip behind `p256`, and of the 16-byte base only c and p are set: every
// entry point below looks at the field on the host before it touches the slab.
struct lfgpu_ligero_prover : lig::Slab<elt_t> {
  int field = 0, k = 0;
  Lig256* p256 = nullptr;
  ~lfgpu_ligero_prover() {
    if (p256) lf_lig256_free(p256);
  }
  // lfgpu_ligero_prove: the write_com_proof bytes between its size query and the copy
  std::vector<uint8_t> wire;
  bool wire_held = false;
};

static size_t ceildiv(size_t a, size_t b) { return (a + b - 1) / b; }
static size_t merkle_tree_len(size_t n) {  // merkle_tree.h:62-70
  size_t r = 1;
  size_t pos = n - 1;
  for (pos += n; pos > 1; pos >>= 1) ++r;
  return r;
}

// LigeroParam::layout (lib/ligero/ligero_param.h:185-295): fills *p for block_enc = e and returns the proof-size
// estimate, or SIZE_MAX where the reference rejects the layout.
static size_t ligero_layout(lfgpu_ligero_param* p, int field, int k, size_t e) {
  const size_t max_lg_size = 28, max_size = (size_t)1 << max_lg_size;
  const size_t field_bytes = field == LFGPU_FIELD_P256 ? 32 : 16;  // Field::kBytes / kSubFieldBytes
  const size_t subfield_bytes = field == LFGPU_FIELD_GF2_128 ? (((size_t)1 << k) / 8) : field_bytes;
  const size_t nw = p->nw, nq = p->nq, rateinv = p->rateinv, nreq = p->nreq;
  p->r = nreq;
  p->block_enc = e;
  size_t subfield_bits = 8 * subfield_bytes;
  if (subfield_bits <= max_lg_size && e >= ((size_t)1 << subfield_bits)) return SIZE_MAX;
  if (e > max_size || rateinv > max_size || (e + 1) < (2 + rateinv)) return SIZE_MAX;
  p->block = (e + 1) / (2 + rateinv);
  if (p->block < p->r) return SIZE_MAX;
  p->w = p->block - p->r;
  if (p->w < p->r) return SIZE_MAX;
  p->dblock = 2 * p->block - 1;
  if (e < p->dblock) return SIZE_MAX;
  p->block_ext = e - p->dblock;
  p->nwrow = ceildiv(nw, p->w);
  p->nqtriples = ceildiv(nq, p->w);
  p->nwqrow = p->nwrow + 3 * p->nqtriples;
  p->nrow = p->nwqrow + 3;
  if (p->nrow >= max_size / e) return SIZE_MAX;
  if (p->block_ext == 0) return SIZE_MAX;  // merkle_commitment_len(0) is undefined; a commitment needs leaves
  p->mc_pathlen = merkle_tree_len(p->block_ext);
  uint64_t sz = 32;                                                     // commitment
  sz += (uint64_t)p->mc_pathlen / 2 * (uint64_t)nreq * 32;             // Merkle openings (approximation)
  sz += (uint64_t)p->block * field_bytes;                              // y_ldt
  sz += (uint64_t)p->dblock * field_bytes;                             // y_dot
  sz += (uint64_t)(p->dblock - p->w) * field_bytes;                    // y_quad
  sz += (uint64_t)nreq * 32;                                           // nonces
  sz += (uint64_t)p->nrow * (uint64_t)nreq * (uint64_t)subfield_bytes; // req
  return (size_t)sz;
}

// block_enc != 0: LigeroParam(nw, nq, rateinv, nreq, block_enc) (ligero_param.h:172-178);
// block_enc == 0: the deprecated ctor that searches block_enc over powers of two for the smallest proof
// (ligero_param.h:152-169; what ZkProof(c, rate, req) and the benchmarks use).
extern "C" int lfgpu_ligero_param_init(lfgpu_ligero_param* p, int field, int k, size_t nw, size_t nq, size_t rateinv,
                                       size_t nreq, size_t block_enc) {
  if (!p) return LFGPU_ERR_ARG;
  memset(p, 0, sizeof(*p));
  p->nw = nw;
  p->nq = nq;
  p->rateinv = rateinv;
  p->nreq = nreq;
  if (block_enc == 0) {
    size_t best = SIZE_MAX, best_e = 1;
    for (size_t e = 1; e <= ((size_t)1 << 28); e *= 2) {
      size_t sz = ligero_layout(p, field, k, e);
      if (sz < best) {
        best = sz;
        best_e = e;
      }
    }
    block_enc = best_e;
  }
  if (ligero_layout(p, field, k, block_enc) == SIZE_MAX) return LFGPU_ERR_ARG;
  if (!(p->block_enc > p->block)) return LFGPU_ERR_ARG;  // sanity(): block_enc > block
  p->ildt = 0;
  p->idot = 1;
  p->iquad = 2;
  p->iw = 3;
  p->iq = p->iw + p->nwrow;
  return LFGPU_OK;
}

int lf_rs_rows(lfgpu_ctx* c, int field, int k, size_t nrow, size_t n, size_t m, elt_t* d, size_t ld) {
  if (nrow == 0) return LFGPU_OK;
  if (field == LFGPU_FIELD_GF2_128) return lfgpu_gf2128_rs_encode_rows(c, k, nrow, n, m, d, ld);
  // Fp128: the 2^32-order root of lib/algebra/fp_p128.h:48-56
  static const char* kOmega = "164956748514267535023998284330560247862";
  unsigned __int128 v = 0;
  for (const char* s = kOmega; *s; ++s) v = v * 10 + (unsigned)(*s - '0');
  elt_t raw{(u64)v, (u64)(v >> 64)};
  elt_t rsq{1, 0};
  for (int i = 0; i < 256; ++i) rsq = fp_add(rsq, rsq);
  elt_t w = fp_mul(raw, rsq);
  uint64_t om[2] = {w.lo, w.hi};
  return lfgpu_fp128_rs_encode_rows(c, nrow, n, m, om, (uint64_t)1 << 32, d, ld);
}

// p256_ok: the entry point also serves Fp256Base (lfgpu_ligero_commit, lfgpu_ligero_layout_rows)
static bool ligero_args_ok(int field, int k, const lfgpu_ligero_param* pp, const void* h_W, const size_t* h_lqc, lfgpu_rng_fn rng, bool p256_ok = false) {
  if (!pp || !rng || (pp->nw && !h_W) || (pp->nq && !h_lqc)) return false;
  if (field == LFGPU_FIELD_P256) return p256_ok;
  if (field != LFGPU_FIELD_GF2_128 && field != LFGPU_FIELD_FP128) return false;
  if (field == LFGPU_FIELD_GF2_128 && k != 4 && k != 5) return false;
  return true;
}

// Multi-GPU commit, host half (no device needed): see include/lfgpu.h
extern "C" int lfgpu_ligero_layout_rows(int field, int k, const lfgpu_ligero_param* pp, const void* h_W, size_t subfield_boundary,
                                        const size_t* h_lqc, lfgpu_rng_fn rng, void* user, size_t row_lo, size_t row_hi, void* h_rows,
                                        uint8_t* h_nonces) {
  if (!ligero_args_ok(field, k, pp, h_W, h_lqc, rng, true) || row_lo > row_hi || row_hi > pp->nrow || (row_hi > row_lo && !h_rows)) return LFGPU_ERR_ARG;
  char err[256];
  if (field == LFGPU_FIELD_P256)
    return lig::layout(lig::Host32{}, *pp, (const elt32_t*)h_W, 0, h_lqc, rng, user, false, row_lo, row_hi, (elt32_t*)h_rows, h_nonces, err);
  GfHostCtx g;
  if (field == LFGPU_FIELD_GF2_128 && !lf_gf_ctx_build(&g, k)) return LFGPU_ERR_ARG;
  return lig::layout(lig::Host16{field, k, &g}, *pp, (const elt_t*)h_W, subfield_boundary, h_lqc, rng, user, false, row_lo, row_hi, (elt_t*)h_rows, h_nonces, err);
}

// ------------------------------------------------------------------ rows sharded over the GPUs of a node
extern "C" int lfgpu_ligero_row_shard(const lfgpu_ligero_param* p, int rank, int world, size_t* row_lo, size_t* row_hi) {
  if (!p || !row_lo || !row_hi || world < 1 || rank < 0 || rank >= world) return LFGPU_ERR_ARG;
  size_t lo, cnt;
  lig::shard_split(p->nrow, rank, world, &lo, &cnt);
  *row_lo = std::min(lo, p->iq);
  *row_hi = rank == world - 1 ? p->nrow : std::min(lo + cnt, p->iq);
  return LFGPU_OK;
}
namespace {
struct RecordRng {  // rank 0: the caller's engine, every byte kept
  lfgpu_rng_fn rng;
  void* user;
  std::vector<uint8_t>* rec;
};
void record_fn(void* u, uint8_t* buf, size_t n) {
  RecordRng* r = (RecordRng*)u;
  r->rng(r->user, buf, n);
  r->rec->insert(r->rec->end(), buf, buf + n);
}
struct ReplayRng {  // every rank: the broadcast stream (running dry yields zeros and sets `dry`)
  const std::vector<uint8_t>* data;
  size_t pos = 0;
  bool dry = false;
};
void replay_fn(void* u, uint8_t* buf, size_t n) {
  ReplayRng* r = (ReplayRng*)u;
  if (r->pos + n > r->data->size()) {
    r->dry = true;
    memset(buf, 0, n);
    return;
  }
  memcpy(buf, r->data->data() + r->pos, n);
  r->pos += n;
}
bool comm_ok(const lfgpu_comm_ops* cm) { return cm && cm->world >= 1 && cm->rank >= 0 && cm->rank < cm->world && cm->all_gather && cm->all_to_all && cm->broadcast; }
}  // namespace
// one rank's byte string to every rank (length first); host buffers
int lf_comm_bcast_blob(const lfgpu_comm_ops* cm, std::vector<uint8_t>& blob) {
  if (cm->world == 1) return LFGPU_OK;
  uint64_t n = cm->rank == 0 ? blob.size() : 0;
  if (cm->broadcast(cm->user, &n, 8, 0, 0, nullptr)) return LFGPU_ERR_HIP;
  if (cm->rank != 0) blob.assign(n, 0);
  if (n && cm->broadcast(cm->user, blob.data(), n, 0, 0, nullptr)) return LFGPU_ERR_HIP;
  return LFGPU_OK;
}
void lf_replay_rng(const std::vector<uint8_t>* data, lfgpu_rng_fn* fn, void** user, void* storage /* >= sizeof(ReplayRng) */) {
  ReplayRng* r = new (storage) ReplayRng{data, 0, false};
  *fn = replay_fn;
  *user = r;
}
void lf_record_rng(lfgpu_rng_fn rng, void* rng_user, std::vector<uint8_t>* rec, lfgpu_rng_fn* fn, void** user, void* storage /* >= sizeof(RecordRng) */) {
  RecordRng* r = new (storage) RecordRng{rng, rng_user, rec};
  *fn = record_fn;
  *user = r;
}
static int layout_sharded_host(const lig::Host16& hp, const lfgpu_ligero_param& p, const void* h_W, size_t subfield_boundary, const size_t* h_lqc,
                               lfgpu_rng_fn rng, void* user, const lfgpu_comm_ops* cm, bool exact, size_t row_lo, size_t row_hi, elt_t* H, uint8_t* nonces,
                               char* err) {
  // the RandomEngine is ONE sequential stream (ligero_prover.h:171-270, merkle_commitment.h:52-54): rank 0 draws all of it
  // (recorded while it lays out its own slab), the other ranks replay it and keep their rows
  std::vector<uint8_t> stream;
  LF_SCRUB_ON_EXIT(stream);
  if (cm->rank == 0) {  // rank 0 lays out its own slab while it draws: one pass, and the others wait for nothing else
    RecordRng rec{rng, user, &stream};
    const int rc = lig::layout(hp, p, (const elt_t*)h_W, subfield_boundary, h_lqc, record_fn, &rec, exact, row_lo, row_hi, H, nonces, err);
    const bool sent = lf_comm_bcast_blob(cm, stream) == LFGPU_OK;  // even after a failed layout: the others are waiting in the broadcast
    if (rc) return rc;
    if (!sent) {
      snprintf(err, 256, "ligero (sharded): broadcast hook failed");
      return LFGPU_ERR_HIP;
    }
    return LFGPU_OK;
  }
  if (lf_comm_bcast_blob(cm, stream)) {
    snprintf(err, 256, "ligero (sharded): broadcast hook failed");
    return LFGPU_ERR_HIP;
  }
  ReplayRng rep{&stream, 0, false};
  const int rc = lig::layout(hp, p, (const elt_t*)h_W, subfield_boundary, h_lqc, replay_fn, &rep, exact, row_lo, row_hi, H, nonces, err);
  if (rc) return rc;
  if (rep.dry || rep.pos != stream.size()) {
    snprintf(err, 256, "ligero (sharded): the replayed random stream does not match the layout (%zu of %zu bytes)", rep.pos, stream.size());
    return LFGPU_ERR_ASSERT;
  }
  return LFGPU_OK;
}
extern "C" int lfgpu_ligero_layout_rows_sharded(int field, int k, const lfgpu_ligero_param* pp, const void* h_W, size_t subfield_boundary,
                                                const size_t* h_lqc, lfgpu_rng_fn rng, void* user, const lfgpu_comm_ops* cm, void* h_rows,
                                                uint8_t* h_nonces) {
  if (!pp || !comm_ok(cm) || (cm->rank == 0 && !rng) || (pp->nw && !h_W) || (pp->nq && !h_lqc)) return LFGPU_ERR_ARG;
  if (field != LFGPU_FIELD_GF2_128 && field != LFGPU_FIELD_FP128) return LFGPU_ERR_ARG;
  GfHostCtx g;
  if (field == LFGPU_FIELD_GF2_128 && !lf_gf_ctx_build(&g, k)) return LFGPU_ERR_ARG;
  size_t lo, hi;
  LF_TRY(lfgpu_ligero_row_shard(pp, cm->rank, cm->world, &lo, &hi));
  if (hi > lo && !h_rows) return LFGPU_ERR_ARG;
  char err[256] = {0};
  return layout_sharded_host(lig::Host16{field, k, &g}, *pp, h_W, subfield_boundary, h_lqc, rng, user, cm, false, lo, hi, (elt_t*)h_rows, h_nonces, err);
}

// host-only check of a caller's hooks
extern "C" int lfgpu_comm_selftest(const lfgpu_comm_ops* cm) {
  if (!comm_ok(cm)) return LFGPU_ERR_ARG;
  const int W = cm->world, r = cm->rank;
  {  // broadcast from every root
    for (int root = 0; root < W; ++root) {
      uint8_t b[37];
      for (int i = 0; i < 37; ++i) b[i] = (uint8_t)(r == root ? 11 * root + i : 0xEE);
      if (cm->broadcast(cm->user, b, 37, root, 0, nullptr)) return LFGPU_ERR_HIP;
      for (int i = 0; i < 37; ++i)
        if (b[i] != (uint8_t)(11 * root + i)) return LFGPU_ERR_ASSERT;
    }
  }
  {  // all_gather
    std::vector<uint8_t> mine(53), all((size_t)53 * W);
    for (int i = 0; i < 53; ++i) mine[i] = (uint8_t)(7 * r + 3 * i);
    if (cm->all_gather(cm->user, mine.data(), all.data(), 53, 0, nullptr)) return LFGPU_ERR_HIP;
    for (int q = 0; q < W; ++q)
      for (int i = 0; i < 53; ++i)
        if (all[(size_t)53 * q + i] != (uint8_t)(7 * q + 3 * i)) return LFGPU_ERR_ASSERT;
  }
  {  // ragged all_to_all: rank p sends 5 + p + 2 q bytes to rank q (zero-length blocks included: p = q = 0 sends 5)
    std::vector<size_t> so(W), sb(W), ro(W), rb(W);
    size_t st = 0, rt = 0;
    for (int q = 0; q < W; ++q) {
      so[q] = st;
      sb[q] = (size_t)(5 + r + 2 * q) * ((r + q) % 3 != 2);
      st += sb[q];
      ro[q] = rt;
      rb[q] = (size_t)(5 + q + 2 * r) * ((q + r) % 3 != 2);
      rt += rb[q];
    }
    std::vector<uint8_t> send(st + 1), recv(rt + 1, 0xEE);
    for (int q = 0; q < W; ++q)
      for (size_t i = 0; i < sb[q]; ++i) send[so[q] + i] = (uint8_t)(r * 31 + q * 17 + i);
    if (cm->all_to_all(cm->user, send.data(), so.data(), sb.data(), recv.data(), ro.data(), rb.data(), 0, nullptr)) return LFGPU_ERR_HIP;
    for (int q = 0; q < W; ++q)
      for (size_t i = 0; i < rb[q]; ++i)
        if (recv[ro[q] + i] != (uint8_t)(q * 31 + r * 17 + i)) return LFGPU_ERR_ASSERT;
  }
  return LFGPU_OK;
}

extern "C" int lfgpu_ligero_free(lfgpu_ligero_prover* pr) {
  if (!pr) return LFGPU_ERR_ARG;
  delete pr;  // ~Slab scrubs the buffers it owns and returns them to the context's pool
  return LFGPU_OK;
}
extern "C" int lfgpu_ligero_tableau(lfgpu_ligero_prover* pr, void** d_T) {
  if (!pr || !d_T) return LFGPU_ERR_ARG;
  *d_T = pr->p256 ? lf_lig256_tableau(pr->p256) : pr->d_T;
  return LFGPU_OK;
}

// y[j] = T0[j] + sum_i A[i][j] * T[i][j]        (dot_proof accumulation, Blas::vaxpy blas.h:71-78)
// Workgroup = 64 columns x 16 row slices (a lane per column alone would be <= 4 workgroups of 150 sequential
// products each: latency-bound); slices are folded through LDS.
// The body of rows_vaxpy_kernel and of rows_combo_batch_kernel.  DOT: the accumulation above over n columns.  LDT: the low-degree
// combination yl[j] = Tl[j] + sum_i u[i] * T[i][j] for j < nl (the body of rows_axpy_kernel, sumcheck.hip, with the blinding row
// added in the fold).  With both set one pass reads every T element once for the two sums (nl <= n; slice 1 folds the second).
template <int F, bool DOT, bool LDT>
__device__ __forceinline__ void rows_combo_body(u32 nrows, size_t n, size_t nl, const elt_t* __restrict__ T0, const elt_t* __restrict__ A, size_t lda,
                                                const elt_t* __restrict__ T, size_t ld, elt_t* __restrict__ y, const elt_t* __restrict__ Tl,
                                                const elt_t* __restrict__ u, elt_t* __restrict__ yl, elt_t (*part)[64], elt_t (*partl)[64]) {
  const u32 col = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const size_t j = (size_t)blockIdx.x * 64 + col;
  elt_t acc = elt_zero(), accl = elt_zero();
  if (j < (DOT ? n : nl))
    for (u32 i = slice; i < nrows; i += 16) {
      const elt_t t = ld16(&T[(size_t)i * ld + j]);
      if (DOT) acc = Fld<F>::add(acc, Fld<F>::mul(t, ld16(&A[(size_t)i * lda + j])));
      if (LDT && j < nl) accl = Fld<F>::add(accl, Fld<F>::mul(t, ld16(&u[i])));
    }
  if (DOT) part[slice][col] = acc;
  if (LDT) partl[slice][col] = accl;
  __syncthreads();
  if (DOT && slice == 0 && j < n) {
    acc = ld16(&T0[j]);
    for (u32 k = 0; k < 16; ++k) acc = Fld<F>::add(acc, part[k][col]);
    st16(&y[j], acc);
  }
  if (LDT && slice == (DOT ? 1 : 0) && j < nl) {
    accl = ld16(&Tl[j]);
    for (u32 k = 0; k < 16; ++k) accl = Fld<F>::add(accl, partl[k][col]);
    st16(&yl[j], accl);
  }
}
template <int F>
__global__ __launch_bounds__(1024) void rows_vaxpy_kernel(u32 nrows, size_t n, const elt_t* __restrict__ T0, const elt_t* __restrict__ A,
                                                          size_t lda, const elt_t* __restrict__ T, size_t ld, elt_t* __restrict__ y) {
  __shared__ elt_t part[16][64];
  rows_combo_body<F, true, false>(nrows, n, 0, T0, A, lda, T, ld, y, nullptr, nullptr, nullptr, part, nullptr);
}
// nb tableaux of one shape (statement blockIdx.y; rows of T_b at the element offsets o_dot / o_ldt / o_w of its base pointer):
//   DOT: y_b[nl + j] = T_b[idot][j] + sum_i Aext_b[i][j] * T_b[iw + i][j]   (j < n = dblock), Aext_b = A + b * sA, lda elements per row
//   LDT: y_b[j]      = T_b[ildt][j] + sum_i u_b[i]       * T_b[iw + i][j]   (j < nl = block), u_b = u + b * su
// with y_b = y + b * sy.  The fused instance <true, true> needs 91 (GF) / 80 (Fp128) VGPRs against the 59 / 40 of rows_vaxpy_kernel:
// one 1024-lane workgroup per CU instead of two, so the prover launches <true, false> and <false, true>.
// Headroom: the Fp128 instances of those two need 61 VGPRs (rows_vaxpy_kernel<FP128>: 40, same body; the cause was not looked for)
// and two 1024-lane workgroups per CU need <= 64.  After a change to rows_combo_body or to this kernel's addressing, read the
// -Rpass-analysis=kernel-resource-usage figures again: three more registers halve the workgroups per CU.
template <int F, bool DOT, bool LDT>
__global__ __launch_bounds__(1024) void rows_combo_batch_kernel(u32 nrows, size_t n, size_t nl, LfBatchPtrs T, size_t ld, size_t o_dot, size_t o_ldt,
                                                                size_t o_w, const elt_t* __restrict__ A, size_t sA, size_t lda,
                                                                const elt_t* __restrict__ u, size_t su, elt_t* __restrict__ y, size_t sy) {
  __shared__ elt_t part[DOT && LDT ? 32 : 16][64];
  const u32 b = blockIdx.y;
  const elt_t* Tb = (const elt_t*)T.p[b];
  elt_t* yb = y + (size_t)b * sy;
  rows_combo_body<F, DOT, LDT>(nrows, n, nl, Tb + o_dot, A + (size_t)b * sA, lda, Tb + o_w, ld, yb + nl, Tb + o_ldt, u + (size_t)b * su, yb, part,
                               DOT && LDT ? part + 16 : part);
}
// y[j] = Tq[j] + sum_i u[i] * (z_i[j] - x_i[j]*y_i[j])   (quadratic_proof :311-333)
// (the body of quad_combo_kernel and of its batched twin)
template <int F>
__device__ __forceinline__ void quad_combo_body(u32 nt, size_t n, const elt_t* __restrict__ Tq, const elt_t* __restrict__ u, const elt_t* __restrict__ X,
                                                const elt_t* __restrict__ Y, const elt_t* __restrict__ Z, size_t ld, elt_t* __restrict__ y) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  elt_t acc = ld16(&Tq[j]);
  for (u32 i = 0; i < nt; ++i) {
    elt_t t = Fld<F>::sub(ld16(&Z[(size_t)i * ld + j]), Fld<F>::mul(ld16(&X[(size_t)i * ld + j]), ld16(&Y[(size_t)i * ld + j])));
    acc = Fld<F>::add(acc, Fld<F>::mul(ld16(&u[i]), t));
  }
  st16(&y[j], acc);
}
template <int F>
__global__ void quad_combo_kernel(u32 nt, size_t n, const elt_t* __restrict__ Tq, const elt_t* __restrict__ u,
                                  const elt_t* __restrict__ X, const elt_t* __restrict__ Y, const elt_t* __restrict__ Z,
                                  size_t ld, elt_t* __restrict__ y) {
  quad_combo_body<F>(nt, n, Tq, u, X, Y, Z, ld, y);
}
// statement blockIdx.y: rows IQUAD (o_quad) and X | Y | Z (nt rows each from o_x) of its own tableau, u_b = u + b * su, y_b = y + b * sy
template <int F>
__global__ void quad_combo_batch_kernel(u32 nt, size_t n, LfBatchPtrs T, size_t ld, size_t o_quad, size_t o_x, const elt_t* __restrict__ u, size_t su,
                                        elt_t* __restrict__ y, size_t sy) {
  const u32 b = blockIdx.y;
  const elt_t* Tb = (const elt_t*)T.p[b];
  const elt_t* X = Tb + o_x;
  const elt_t* Y = X + (size_t)nt * ld;
  quad_combo_body<F>(nt, n, Tb + o_quad, u + (size_t)b * su, X, Y, Y + (size_t)nt * ld, ld, y + (size_t)b * sy);
}
// Aext[i] = [0^r | A[i*w .. (i+1)*w) | 0...]   (layout_Aext ligero_param.h:423-430)
__global__ void layout_aext_kernel(u32 r, u32 w, size_t lda, const elt_t* __restrict__ A, elt_t* __restrict__ Aext) {
  u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  u32 i = blockIdx.y;
  if (j >= r + w) return;
  st16(&Aext[(size_t)i * lda + j], j < r ? elt_zero() : ld16(&A[(size_t)i * w + (j - r)]));
}

#define LIG_DISPATCH(field, KERNEL, grid, block, ...)                                  \
  do {                                                                                 \
    if ((field) == LFGPU_FIELD_GF2_128)                                                \
      hipLaunchKernelGGL(KERNEL<FIELD_GF2_128>, grid, block, 0, c->stream, __VA_ARGS__); \
    else                                                                               \
      hipLaunchKernelGGL(KERNEL<FIELD_FP128>, grid, block, 0, c->stream, __VA_ARGS__);   \
  } while (0)

// ---- the kernels of the inner-product matrix (lig::a_rows, ligero_slab.h)
// (the bodies of the two kernels and of their batched twins: flat position t of n; nflat = nrows * w bounds the sparse indices)
template <int F>
__device__ __forceinline__ void a_rows_dense_body(u32 r, u32 w, size_t ld, elt_t scale, const elt_t* __restrict__ dense, size_t n, elt_t* __restrict__ rows) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const size_t i = t / w, j = t % w;
  st16(&rows[i * ld + r + j], Fld<F>::mul(scale, ld16(&dense[t])));
}
template <int F>
__device__ __forceinline__ void a_rows_sparse_body(u32 r, u32 w, size_t ld, const u64* __restrict__ idx, const elt_t* __restrict__ val, size_t n, size_t nflat,
                                                   elt_t* __restrict__ rows) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const u64 f = idx[t];
  if (f >= nflat) return;
  const size_t i = f / w, j = f % w;
  elt_t* dst = &rows[i * ld + r + j];
  st16(dst, Fld<F>::add(ld16(dst), ld16(&val[t])));
}
template <int F>
__global__ void a_rows_dense_kernel(u32 r, u32 w, size_t ld, elt_t scale, const elt_t* __restrict__ dense, size_t n,
                                    elt_t* __restrict__ rows) {
  a_rows_dense_body<F>(r, w, ld, scale, dense, n, rows);
}
template <int F>
__global__ void a_rows_sparse_kernel(u32 r, u32 w, size_t ld, const u64* __restrict__ idx, const elt_t* __restrict__ val, size_t n, size_t nflat,
                                     elt_t* __restrict__ rows) {
  a_rows_sparse_body<F>(r, w, ld, idx, val, n, nflat, rows);
}
// statement blockIdx.y: rows_b = rows + b * srows.  Dense: rows_b[i][r + j] = scale[b] * dense_b[t] with dense_b a per-statement pointer.
// Sparse: the statements' (idx, val) lists stand one after the other; statement b's are entries [off[b], off[b + 1]) (possibly none).
template <int F>
__global__ void a_rows_dense_batch_kernel(u32 r, u32 w, size_t ld, const elt_t* __restrict__ scale, LfBatchPtrs dense, size_t n, elt_t* __restrict__ rows,
                                          size_t srows) {
  const u32 b = blockIdx.y;
  a_rows_dense_body<F>(r, w, ld, ld16(&scale[b]), (const elt_t*)dense.p[b], n, rows + (size_t)b * srows);
}
template <int F>
__global__ void a_rows_sparse_batch_kernel(u32 r, u32 w, size_t ld, const u64* __restrict__ idx, const elt_t* __restrict__ val, const u64* __restrict__ off,
                                           size_t nflat, elt_t* __restrict__ rows, size_t srows) {
  const u32 b = blockIdx.y;
  const u64 o = off[b];
  a_rows_sparse_body<F>(r, w, ld, idx + o, val + o, (size_t)(off[b + 1] - o), nflat, rows + (size_t)b * srows);
}

// ---- inner_product_vector from the caller's term list (LigeroCommon::inner_product_vector, ligero_param.h:382-421): terms in any
// order, duplicates allowed, one wire read by thousands of terms the normal case.  The sums go into accumulators indexed by the
// flat position f = i * w + j of A (not into the strided rows): two 64-bit words per entry and atomic XOR for GF(2^128); four
// 64-bit sums of 32-bit limbs and atomic adds for Fp128 (integer sums of residues, < 2^32 summands per entry, one
// fp_reduce_limbs pass: the pattern of bindg_emit_fp_kernel, quad.hip).  Both are exact and independent of arrival order.  Runs of
// equal targets in lane order are folded before the atomics: in the block for GF (runfold.h), in the wave for Fp128.
struct llterm_t {  // the memory image of lfgpu_ligero_llterm
  u64 c, w;
  elt_t k;
};
static_assert(sizeof(llterm_t) == 32 && sizeof(lfgpu_ligero_llterm) == 32 && sizeof(size_t) == 8, "lfgpu_ligero_llterm is uploaded as it stands");
#define AT_THREADS 256
#define AT_BLOCKS_MAX 1024  // grid stride: AT_THREADS * AT_BLOCKS_MAX terms per sweep
__global__ __launch_bounds__(AT_THREADS) void a_terms_gf_kernel(size_t n, const llterm_t* __restrict__ t, const elt_t* __restrict__ alphal,
                                                                u64* __restrict__ acc) {
  const size_t stride = (size_t)gridDim.x * AT_THREADS;
  for (size_t base = (size_t)blockIdx.x * AT_THREADS; base < n; base += stride) {  // block-uniform trip count: the fold has barriers
    const size_t i = base + threadIdx.x;
    u32 key = 0xffffffffu;
    elt_t v = elt_zero();
    if (i < n) {
      const llterm_t e = t[i];
      key = (u32)e.w;
      v = gf_mul(e.k, ld16(&alphal[e.c]));
    }
    gf_run_fold_commit<AT_THREADS>(key, v, acc);
  }
}
__global__ __launch_bounds__(AT_THREADS) void a_terms_fp_kernel(size_t n, const llterm_t* __restrict__ t, const elt_t* __restrict__ alphal,
                                                                u64* __restrict__ acc) {
  const size_t stride = (size_t)gridDim.x * AT_THREADS;
  const u32 lane = threadIdx.x & 63;
  for (size_t base = (size_t)blockIdx.x * AT_THREADS; base < n; base += stride) {  // wave-uniform trip count: the fold shuffles
    const size_t i = base + threadIdx.x;
    u32 key = 0xffffffffu;
    u64 l0 = 0, l1 = 0, l2 = 0, l3 = 0;
    if (i < n) {
      const llterm_t e = t[i];
      key = (u32)e.w;
      const elt_t v = fp_mul(e.k, ld16(&alphal[e.c]));
      l0 = (u32)v.lo;
      l1 = v.lo >> 32;
      l2 = (u32)v.hi;
      l3 = v.hi >> 32;
    }
    // segmented suffix sums over the wave's runs of equal keys (run id = number of run heads at or before the lane, as runfold.h);
    // a run's head lane ends with the run's limb sums, < 64 * 2^32 each
    const u32 pkey = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || pkey != key;
    const u64 hmask = __ballot(head);
    const u32 rid = (u32)__popcll(hmask & ((2ull << lane) - 1));
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u64 o0 = __shfl_down(l0, off, 64), o1 = __shfl_down(l1, off, 64), o2 = __shfl_down(l2, off, 64), o3 = __shfl_down(l3, off, 64);
      const u32 orid = __shfl_down(rid, off, 64);
      if (lane + off < 64 && orid == rid) {
        l0 += o0;
        l1 += o1;
        l2 += o2;
        l3 += o3;
      }
    }
    if (head && key != 0xffffffffu) {
      u64* a = acc + 4 * (size_t)key;
      atomicAdd(&a[0], l0);
      atomicAdd(&a[1], l1);
      atomicAdd(&a[2], l2);
      atomicAdd(&a[3], l3);
    }
  }
}
template <int F>
__device__ __forceinline__ void a_terms_acc(u64* __restrict__ acc, u64 f, elt_t v) {
  if (F == FIELD_GF2_128) {
    atomicXor(&acc[2 * f], v.lo);
    atomicXor(&acc[2 * f + 1], v.hi);
  } else {
    atomicAdd(&acc[4 * f], (u64)(u32)v.lo);
    atomicAdd(&acc[4 * f + 1], v.lo >> 32);
    atomicAdd(&acc[4 * f + 2], (u64)(u32)v.hi);
    atomicAdd(&acc[4 * f + 3], v.hi >> 32);
  }
}
// the quadratic copy constraints: A[a0 + j * step + iw] += aq, A[lqc[iw][j]] -= aq for aq = alphaq[iw][j], j < 3
template <int F>
__global__ void a_terms_quad_kernel(u32 n3 /* 3 nq */, const u64* __restrict__ lqc, const elt_t* __restrict__ alphaq, u64 a0, u64 step, u64* __restrict__ acc) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n3) return;
  const u32 iw = t / 3, j = t % 3;
  const elt_t aq = ld16(&alphaq[t]);
  a_terms_acc<F>(acc, a0 + (u64)j * step + iw, aq);
  a_terms_acc<F>(acc, lqc[t], Fld<F>::sub(elt_zero(), aq));
}
// rows[i][r + j] += the sum standing in the accumulators of flat position i * w + j
template <int F>
__global__ void a_terms_finish_kernel(u32 r, u32 w, size_t ld, size_t nflat, const u64* __restrict__ acc, elt_t* __restrict__ rows) {
  const size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nflat) return;
  const elt_t v = F == FIELD_GF2_128 ? elt_t{acc[2 * f], acc[2 * f + 1]} : fp_reduce_limbs(acc[4 * f], acc[4 * f + 1], acc[4 * f + 2], acc[4 * f + 3]);
  elt_t* dst = &rows[(f / w) * ld + r + f % w];
  st16(dst, Fld<F>::add(ld16(dst), v));
}

// ---- the width policy of ligero_slab.h for the two 16-byte fields: it wraps the entry points and kernels that exist and carries
// the field.  These steps upload their host vectors themselves: lfgpu_rows_axpy and lfgpu_gather_columns end with a synchronise,
// a short sparse list goes through the pinned staging ring without one.
struct L16 : lig::Host16 {
  int rows_axpy(lfgpu_ctx* c, size_t nrows, size_t n, E* d_y, const E* h_u, const E* d_T, size_t ld) const {
    return lfgpu_rows_axpy(c, field, nrows, n, d_y, (const uint64_t*)h_u, d_T, ld);
  }
  int rows_vaxpy(lfgpu_ctx* c, size_t nrows, size_t n, const E* T0, const E* A, size_t lda, const E* T, size_t ld, E* y) const {
    LIG_DISPATCH(field, rows_vaxpy_kernel, dim3((u32)((n + 63) / 64)), dim3(1024), (u32)nrows, n, T0, A, lda, T, ld, y);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  int quad_combo(lfgpu_ctx* c, size_t nt, size_t n, const E* Tq, const E* u, const E* X, const E* Y, const E* Z, size_t ld, E* y) const {
    LIG_DISPATCH(field, quad_combo_kernel, dim3((u32)((n + 255) / 256)), dim3(256), (u32)nt, n, Tq, u, X, Y, Z, ld, y);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  // lfgpu_ligero_inner_product_rows promises its callers, who bring their own buffer, that the first r + w columns are cleared
  int a_rows_clear(lfgpu_ctx* c, E* d_rows, size_t ld, size_t ncols, size_t nrows) const {
    LF_HIP(c, hipMemset2DAsync(d_rows, ld * 16, 0, ncols * 16, nrows, c->stream));
    return LFGPU_OK;
  }
  int a_rows_dense(lfgpu_ctx* c, size_t r, size_t w, size_t ld, const E& scale, const E* d_dense, size_t n, E* d_rows) const {
    LIG_DISPATCH(field, a_rows_dense_kernel, dim3((u32)((n + 255) / 256)), dim3(256), (u32)r, (u32)w, ld, scale, d_dense, n, d_rows);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  int a_rows_sparse(lfgpu_ctx* c, size_t r, size_t w, size_t ld, const uint64_t* h_idx, const E* h_val, size_t n, size_t nflat, E* d_rows) const {
    void* d_sp = nullptr;
    LF_TRY(lf_scratch2(c, n * 24 + 64, &d_sp));
    E* d_val = (E*)d_sp;
    u64* d_idx = (u64*)(d_val + n);
    if (n * 24 <= LF_STAGE_SLOT) {  // one staged copy: values then indices
      std::vector<uint8_t> pack(n * 24);
      memcpy(pack.data(), h_val, n * 16);
      memcpy(pack.data() + n * 16, h_idx, n * 8);
      LF_TRY(lf_stage_upload(c, d_sp, pack.data(), pack.size()));
    } else {
      LF_HIP(c, hipMemcpyAsync(d_val, h_val, n * 16, hipMemcpyHostToDevice, c->stream));
      LF_HIP(c, hipMemcpyAsync(d_idx, h_idx, n * 8, hipMemcpyHostToDevice, c->stream));
      LF_HIP(c, hipStreamSynchronize(c->stream));
    }
    LIG_DISPATCH(field, a_rows_sparse_kernel, dim3((u32)((n + 255) / 256)), dim3(256), (u32)r, (u32)w, ld, (const u64*)d_idx, (const E*)d_val, n, nflat, d_rows);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  // inner_product_vector from an unsorted term list with duplicates (the kernels above), added to what stands in the rows.
  // The accumulators, the term list (one copy, as the caller holds it) and the challenges (one packed copy) live in scratch2.
  int a_rows_terms(lfgpu_ctx* c, const lfgpu_ligero_param& p, size_t ld, const LfLigeroTerms& t, E* d_rows) const {
    const bool gf = field == LFGPU_FIELD_GF2_128;
    const size_t nflat = p.nwqrow * p.w, n3 = 3 * p.nq, acc_bytes = nflat * (gf ? 16 : 32);
    const size_t small_bytes = (t.nl + n3) * 16 + n3 * 8;
    void* d = nullptr;
    LF_TRY(lf_scratch2(c, acc_bytes + t.nterm * 32 + small_bytes + 64, &d));
    u64* d_acc = (u64*)d;
    llterm_t* d_term = (llterm_t*)((uint8_t*)d + acc_bytes);
    E* d_alphal = (E*)(d_term + t.nterm);
    E* d_alphaq = d_alphal + t.nl;
    u64* d_lqc = (u64*)(d_alphaq + n3);
    LF_HIP(c, hipMemsetAsync(d_acc, 0, acc_bytes, c->stream));
    if (t.nterm) LF_HIP(c, hipMemcpyAsync(d_term, t.term, t.nterm * 32, hipMemcpyHostToDevice, c->stream));
    if (small_bytes) {
      std::vector<uint8_t> pack(small_bytes);
      if (t.nl) memcpy(pack.data(), t.alphal, t.nl * 16);
      if (n3) memcpy(pack.data() + t.nl * 16, t.alphaq, n3 * 16);
      if (n3) memcpy(pack.data() + (t.nl + n3) * 16, t.lqc, n3 * 8);
      if (small_bytes <= LF_STAGE_SLOT) {
        LF_TRY(lf_stage_upload(c, d_alphal, pack.data(), small_bytes));
      } else {
        LF_HIP(c, hipMemcpyAsync(d_alphal, pack.data(), small_bytes, hipMemcpyHostToDevice, c->stream));
        LF_HIP(c, hipStreamSynchronize(c->stream));
      }
    }
    if (t.nterm) {
      const dim3 grid((u32)std::min<size_t>((t.nterm + AT_THREADS - 1) / AT_THREADS, AT_BLOCKS_MAX));
      if (gf) hipLaunchKernelGGL(a_terms_gf_kernel, grid, dim3(AT_THREADS), 0, c->stream, t.nterm, (const llterm_t*)d_term, (const E*)d_alphal, d_acc);
      else hipLaunchKernelGGL(a_terms_fp_kernel, grid, dim3(AT_THREADS), 0, c->stream, t.nterm, (const llterm_t*)d_term, (const E*)d_alphal, d_acc);
      LF_HIP(c, hipGetLastError());
    }
    if (n3) {
      LIG_DISPATCH(field, a_terms_quad_kernel, dim3((u32)((n3 + 255) / 256)), dim3(256), (u32)n3, (const u64*)d_lqc, (const E*)d_alphaq, (u64)(p.nwrow * p.w),
                   (u64)(p.nqtriples * p.w), d_acc);
      LF_HIP(c, hipGetLastError());
    }
    LIG_DISPATCH(field, a_terms_finish_kernel, dim3((u32)((nflat + 255) / 256)), dim3(256), (u32)p.r, (u32)p.w, ld, nflat, (const u64*)d_acc, d_rows);
    LF_HIP(c, hipGetLastError());
    // the term list is the caller's memory: its upload is over before this returns
    LF_HIP(c, hipStreamSynchronize(c->stream));
    return LFGPU_OK;
  }
  int gather_columns(lfgpu_ctx* c, size_t nrow, size_t ld, size_t col0, const E* d_T, const size_t* h_idx, size_t nreq, E* d_req) const {
    return lfgpu_gather_columns(c, nrow, ld, col0, d_T, h_idx, nreq, d_req);
  }
  int rs_rows(lfgpu_ctx* c, size_t nrow, size_t n, size_t m, E* d, size_t ld) const { return lf_rs_rows(c, field, k, nrow, n, m, d, ld); }
  // GF(2^128) has the one-launch kernel (rows up to the LDS-resident size); Fp128 goes group by group
  int rs_rows_mixed(lfgpu_ctx* c, size_t nrow, size_t n1, size_t n2, size_t lo2, size_t hi2, size_t m, E* d, size_t ld) const {
    return field == LFGPU_FIELD_GF2_128 ? lf_gf_rs_rows_mixed(c, k, nrow, n1, n2, lo2, hi2, m, d, ld) : (int)LFGPU_ERR_UNSUPPORTED;
  }
  int column_leaves(lfgpu_ctx* c, size_t nrow, size_t ld, size_t col0, size_t ncols, const void* d_T, const void* d_nonces, void* d_out) const {
    return lfgpu_column_leaves(c, field, nrow, ld, col0, ncols, d_T, d_nonces, d_out);
  }
  // ---- the steps of lig::prove_batch / open_batch over cb statements (statement blockIdx.y of the batch kernels above)
  // what the batch asks of 16-byte provers beyond lig::batch_core; a borrowed full-range slab will do
  static int batch_ok(lfgpu_ctx* c, const char* who, lfgpu_ligero_prover* const* pr, size_t nb, L16* pol) {
    for (size_t b = 0; b < nb; ++b)
      if (pr[b]->field != pr[0]->field || pr[b]->k != pr[0]->k) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu has another field than prover 0", who, b);
    if (pr[0]->field != LFGPU_FIELD_GF2_128 && pr[0]->field != LFGPU_FIELD_FP128)
      return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "%s: 16-byte fields only (Fp256Base provers take lfgpu_ligero_prove_batch256 / lfgpu_ligero_open_batch256)", who);
    for (size_t b = 0; b < nb; ++b)
      if (pr[b]->sharded || pr[b]->row_lo != 0 || pr[b]->row_hi != pr[b]->p.nrow || !pr[b]->d_T)
        return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "%s: prover %zu is sharded or holds a slab (the batch runs whole tableaux on one GPU)", who, b);
    *pol = L16{{pr[0]->field, pr[0]->k, nullptr}};
    return LFGPU_OK;
  }
  // Fp128: the rows of a chain's extension fit one launch (lf_fp_rs_rows_batch) and its convolution scratch stays below the cap
  size_t batch_rs_cap(const lfgpu_ligero_param& p) const {
    if (field != LFGPU_FIELD_FP128 || !p.nwqrow) return SIZE_MAX;
    size_t P = 1;
    while (P < p.dblock) P <<= 1;
    return std::min<size_t>(65535 / p.nwqrow, LF_CB_SCRATCH_CAP / (p.nwqrow * P * 16));
  }
  int a_rows_dense_batch(lfgpu_ctx* c, size_t cb, size_t r, size_t w, size_t ld, const E* d_scale, const LfBatchPtrs& dense, size_t n, E* d_rows, size_t srows) const {
    LIG_DISPATCH(field, a_rows_dense_batch_kernel, dim3((u32)((n + 255) / 256), (u32)cb), dim3(256), (u32)r, (u32)w, ld, d_scale, dense, n, d_rows, srows);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  int a_rows_sparse_batch(lfgpu_ctx* c, size_t cb, size_t r, size_t w, size_t ld, const u64* d_idx, const E* d_val, const u64* d_off, size_t maxn, size_t nflat,
                          E* d_rows, size_t srows) const {
    LIG_DISPATCH(field, a_rows_sparse_batch_kernel, dim3((u32)((maxn + 255) / 256), (u32)cb), dim3(256), (u32)r, (u32)w, ld, d_idx, d_val, d_off, nflat, d_rows, srows);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  // one launch for the chain; rows longer than the LDS-resident kernel / more rows than a launch takes: statement by statement
  int rs_rows_batch(lfgpu_ctx* c, size_t cb, E* d_rows, size_t srows, size_t nrow, size_t n, size_t m, size_t ld) const {
    E* rows[LFGPU_SC_BATCH_MAX];
    for (size_t b = 0; b < cb; ++b) rows[b] = d_rows + b * srows;
    int rc = LFGPU_ERR_UNSUPPORTED;
    if (field == LFGPU_FIELD_GF2_128) rc = lf_gf_rs_rows_mixed_batch(c, k, cb, rows, nrow, n, n, 0, 0, m, ld);
    else if (cb * nrow <= 65535) rc = lf_fp_rs_rows_batch(c, cb, rows, 0, nrow, n, m, ld);
    if (rc != LFGPU_ERR_UNSUPPORTED) return rc;
    for (size_t b = 0; b < cb; ++b) LF_TRY(rs_rows(c, nrow, n, m, rows[b], ld));
    return LFGPU_OK;
  }
  // the dot proof and the low-degree proof as two launches: see rows_combo_batch_kernel
  template <bool DOT, bool LDT>
  void rows_combo_launch(lfgpu_ctx* c, size_t cb, const lfgpu_ligero_param& p, const LfBatchPtrs& T, const E* A, size_t sA, const E* u, E* y, size_t sy) const {
    const size_t ld = p.block_enc;
    const dim3 grid((u32)(((DOT ? p.dblock : p.block) + 63) / 64), (u32)cb);
    if (field == LFGPU_FIELD_GF2_128)
      hipLaunchKernelGGL((rows_combo_batch_kernel<FIELD_GF2_128, DOT, LDT>), grid, dim3(1024), 0, c->stream, (u32)p.nwqrow, p.dblock, p.block, T, ld, p.idot * ld,
                         p.ildt * ld, p.iw * ld, A, sA, p.dblock, u, p.nwqrow, y, sy);
    else
      hipLaunchKernelGGL((rows_combo_batch_kernel<FIELD_FP128, DOT, LDT>), grid, dim3(1024), 0, c->stream, (u32)p.nwqrow, p.dblock, p.block, T, ld, p.idot * ld,
                         p.ildt * ld, p.iw * ld, A, sA, p.dblock, u, p.nwqrow, y, sy);
  }
  int rows_combo_batch(lfgpu_ctx* c, size_t cb, const lfgpu_ligero_param& p, const LfBatchPtrs& T, const E* A, size_t sA, const E* u, E* y, size_t sy) const {
    rows_combo_launch<true, false>(c, cb, p, T, A, sA, u, y, sy);
    rows_combo_launch<false, true>(c, cb, p, T, A, sA, u, y, sy);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  int quad_combo_batch(lfgpu_ctx* c, size_t cb, const lfgpu_ligero_param& p, const LfBatchPtrs& T, const E* u, E* y, size_t sy) const {
    const size_t ld = p.block_enc;
    LIG_DISPATCH(field, quad_combo_batch_kernel, dim3((u32)((p.dblock + 255) / 256), (u32)cb), dim3(256), (u32)p.nqtriples, p.dblock, T, ld, p.iquad * ld, p.iq * ld, u,
                 p.nqtriples, y, sy);
    LF_HIP(c, hipGetLastError());
    return LFGPU_OK;
  }
  int gather_columns_batch(lfgpu_ctx* c, size_t cb, size_t nrow, size_t ld, size_t col0, const LfBatchPtrs& T, const u64* d_idx, size_t nreq, E* d_req) const {
    return lf_gather_columns_batch(c, cb, nrow, ld, col0, T, d_idx, nreq, d_req);
  }
};
static L16 policy16(const lfgpu_ligero_prover* pr) { return L16{{pr->field, pr->k, nullptr}}; }
// ... for a commit: with the subfield tables of the host layout (null for an unknown k)
static L16 policy16(lfgpu_ctx* c, int field, int k) { return L16{{field, k, field == LFGPU_FIELD_GF2_128 ? lf_gf_ctx(c, k) : nullptr}}; }
static lfgpu_ligero_prover* new_prover16(lfgpu_ctx* c, int field, int k, const lfgpu_ligero_param& p, const lfgpu_comm_ops* cm) {
  lfgpu_ligero_prover* pr = new lfgpu_ligero_prover();
  pr->init(c, p, cm);
  pr->field = field;
  pr->k = k;
  return pr;
}

extern "C" int lfgpu_ligero_encode_rows(lfgpu_ctx* c, int field, int k, const lfgpu_ligero_param* pp, size_t row_lo, size_t row_hi,
                                        const void* h_rows, void* d_slab) {
  if (!c || !pp || row_lo > row_hi || row_hi > pp->nrow || (row_hi > row_lo && (!h_rows || !d_slab)))
    return lf_fail(c, LFGPU_ERR_ARG, "ligero_encode_rows: bad argument");
  if (field != LFGPU_FIELD_GF2_128 && field != LFGPU_FIELD_FP128) return lf_fail(c, LFGPU_ERR_ARG, "ligero_encode_rows: field");
  if (field == LFGPU_FIELD_GF2_128 && !lf_gf_ctx(c, k)) return lf_fail(c, LFGPU_ERR_ARG, "ligero_encode_rows: subfield_log_bits must be 4 or 5");
  LF_HIP(c, hipSetDevice(c->device));
  if (row_hi > row_lo)
    LF_HIP(c, hipMemcpy2DAsync(d_slab, pp->block_enc * 16, h_rows, pp->dblock * 16, pp->dblock * 16, row_hi - row_lo, hipMemcpyHostToDevice, c->stream));
  const int rc = lig::extend_slab(c, policy16(c, field, k), *pp, row_lo, row_hi, (elt_t*)d_slab);
  LF_HIP(c, hipStreamSynchronize(c->stream));  // h_rows is the caller's: the upload must be over before we return
  return rc;
}

// the single-GPU commit is the slab [0, nrow) of the sharded one
extern "C" int lfgpu_ligero_commit(lfgpu_ctx* c, int field, int k, const lfgpu_ligero_param* pp, const void* h_W,
                                   size_t subfield_boundary, const size_t* h_lqc, lfgpu_rng_fn rng, void* user,
                                   uint8_t root_out[32], lfgpu_ligero_prover** out) {
  if (!c || !root_out || !out || !ligero_args_ok(field, k, pp, h_W, h_lqc, rng, true))
    return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit: bad argument (null pointer, field or subfield_log_bits)");
  const lfgpu_ligero_param& p = *pp;
  LF_HIP(c, hipSetDevice(c->device));
  if (field == LFGPU_FIELD_P256) {  // the 32-byte record and its policy are zk256.hip's
    std::unique_ptr<lfgpu_ligero_prover> pr(new lfgpu_ligero_prover());
    pr->c = c;
    pr->p = p;
    pr->field = field;
    LF_TRY(lf_lig256_commit(c, pp, h_W, h_lqc, rng, user, root_out, &pr->p256));
    *out = pr.release();
    return LFGPU_OK;
  }
  const L16 pol = policy16(c, field, k);
  const double t0 = lig::clock_ms();
  std::unique_ptr<lfgpu_ligero_prover> pr(new_prover16(c, field, k, p, nullptr));
  std::vector<elt_t> H(p.nrow * p.dblock);
  LF_SCRUB_ON_EXIT(H);
  char err[256] = {0};
  const int rc = lig::layout(pol, p, (const elt_t*)h_W, subfield_boundary, h_lqc, rng, user, c->rng_exact != 0, 0, p.nrow, H.data(), pr->nonces.data(), err);
  if (rc) return lf_fail(c, rc, "%s", err);
  LF_TRY(lig::commit_rows(pr.get(), pol, H.data(), t0, root_out));
  *out = pr.release();
  return LFGPU_OK;
}

// ------------------------------------------------------------------ nb commits of one shape in one chain of dispatches
// statements per launch chain of the batched RS encode: the Fp128 kernels carry the rows of a group on gridDim.y (<= 65535) and
// the convolution scratch is nb * rows * P * 16 bytes (<= LF_CB_SCRATCH_CAP); LFGPU_CB_CHUNK overrides (read once)
static size_t commit_batch_chunk(int field, const lfgpu_ligero_param& p, size_t nb) {
  static const long env = getenv("LFGPU_CB_CHUNK") ? atol(getenv("LFGPU_CB_CHUNK")) : 0;
  size_t chunk = nb;
  if (field == LFGPU_FIELD_FP128) {
    const size_t g_lo = std::min(p.idot, p.iquad), g_hi = std::max(p.idot, p.iquad) + 1;
    const size_t rows = std::max<size_t>(1, std::max(std::max(g_lo, g_hi - g_lo), p.nrow - g_hi));  // the largest row group
    size_t P = 1;
    while (P < p.block_enc) P <<= 1;
    chunk = std::min(chunk, std::min<size_t>(65535 / rows, LF_CB_SCRATCH_CAP / (rows * P * 16)));
  }
  if (env > 0) chunk = std::min(chunk, (size_t)env);
  return std::max<size_t>(chunk, 1);
}
// the RS extension of nb tableaux whose un-encoded images are on the device
static int ligero_extend_batch(lfgpu_ctx* c, const L16& pol, const lfgpu_ligero_param& p, size_t nb, elt_t* const* d_T) {
  const int field = pol.field, k = pol.k;
  const size_t ld = p.block_enc;
  const size_t lo2 = std::min(p.idot, p.iquad), hi2 = std::max(p.idot, p.iquad) + 1;
  if (hi2 - lo2 != 2) return lf_fail(c, LFGPU_ERR_ARG, "ligero: IDOT and IQUAD rows must be adjacent");
  const size_t chunk = commit_batch_chunk(field, p, nb);
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t cb = std::min(chunk, nb - b0);
    if (field == LFGPU_FIELD_GF2_128) {
      const int rc = lf_gf_rs_rows_mixed_batch(c, k, cb, d_T + b0, p.nrow, p.block, p.dblock, lo2, hi2, p.block_enc, ld);
      if (rc != LFGPU_ERR_UNSUPPORTED) {
        LF_TRY(rc);
        continue;
      }
      // rows longer than the LDS-resident kernel: the single path's encoder, statement by statement
      for (size_t b = b0; b < b0 + cb; ++b) LF_TRY(lig::extend_slab(c, pol, p, 0, p.nrow, d_T[b]));
    } else if (cb * std::max(hi2, p.nrow - hi2) > 65535) {  // (cb = 1) a row group of one statement overflows a launch: the single path's encoder
      for (size_t b = b0; b < b0 + cb; ++b) LF_TRY(lig::extend_slab(c, pol, p, 0, p.nrow, d_T[b]));
    } else {
      LF_TRY(lf_fp_rs_rows_batch(c, cb, d_T + b0, 0, lo2, p.block, p.block_enc, ld));
      LF_TRY(lf_fp_rs_rows_batch(c, cb, d_T + b0, lo2, hi2 - lo2, p.dblock, p.block_enc, ld));
      LF_TRY(lf_fp_rs_rows_batch(c, cb, d_T + b0, hi2, p.nrow - hi2, p.block, p.block_enc, ld));
    }
  }
  return LFGPU_OK;
}

extern "C" int lfgpu_ligero_commit_batch(lfgpu_ctx* c, int field, int k, const lfgpu_ligero_param* pp, size_t nb, const void* const* h_W,
                                         size_t subfield_boundary, const size_t* h_lqc, const lfgpu_rng_fn* rng, void* const* rng_user,
                                         uint8_t* roots_out, lfgpu_ligero_prover** out) {
  if (!c || !pp || !h_W || !rng || !roots_out || !out) return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit_batch: null argument");
  if (nb == 0 || nb > LFGPU_SC_BATCH_MAX) return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit_batch: nb = %zu, a batch holds 1..%d statements", nb, LFGPU_SC_BATCH_MAX);
  for (size_t b = 0; b < nb; ++b)
    if (!ligero_args_ok(field, k, pp, h_W[b], h_lqc, rng[b]))
      return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit_batch: bad argument for statement %zu (null pointer, field or subfield_log_bits)", b);
  for (size_t b = 0; b < nb; ++b) out[b] = nullptr;
  auto user = [&](size_t b) { return rng_user ? rng_user[b] : nullptr; };
  auto drop = [&](int rc) {  // no prover is returned: their buffers go back to the pool scrubbed (lfgpu_ligero_free)
    for (size_t b = 0; b < nb; ++b) {
      if (out[b]) lfgpu_ligero_free(out[b]);
      out[b] = nullptr;
    }
    return rc;
  };
  static const int batched = getenv("LFGPU_COMMIT_BATCH") ? atoi(getenv("LFGPU_COMMIT_BATCH")) : 1;
  if (!batched) {  // the A/B switch: the same semantics over the single-statement device path
    for (size_t b = 0; b < nb; ++b) {
      const int rc = lfgpu_ligero_commit(c, field, k, pp, h_W[b], subfield_boundary, h_lqc, rng[b], user(b), roots_out + 32 * b, &out[b]);
      if (rc) {
        out[b] = nullptr;
        return drop(rc);
      }
    }
    return LFGPU_OK;
  }
  const L16 pol = policy16(c, field, k);
  const lfgpu_ligero_param& p = *pp;
  const size_t ld = p.block_enc, hw = p.dblock, ncols = p.block_ext;
  LF_HIP(c, hipSetDevice(c->device));
  static const bool verbose = getenv("LFGPU_VERBOSE") != nullptr;
  const double tv0 = lig::clock_ms();
  // pinned staging: [nb][nrow][dblock] un-encoded images, then [nb][ncols][32] nonces.  The uploads of the previous call are
  // over (every call ends with a stream synchronise), so the memory may be rewritten at once.
  const size_t img = p.nrow * hw * 16, used = nb * (img + ncols * 32);
  uint8_t* stage = nullptr;
  LF_TRY(lig::cb_stage(c, "ligero_commit_batch", used, &stage));
  uint8_t* const h_non = stage + nb * img;
  const lig::CbScrub scrub{stage, used};
  // the host half, statement by statement in index order: all draws of statement b from rng[b]
  for (size_t b = 0; b < nb; ++b) {
    char err[256] = {0};
    const int rc = lig::layout(pol, p, (const elt_t*)h_W[b], subfield_boundary, h_lqc, rng[b], user(b), c->rng_exact != 0, 0, p.nrow, (elt_t*)(stage + b * img),
                               h_non + b * ncols * 32, err);
    if (rc) return lf_fail(c, rc, "%s (statement %zu)", err, b);
  }
  const double tv1 = lig::clock_ms();
  // After a failed enqueue the stream may still read the staging memory: wait before it is scrubbed
  auto fail = [&](int rc) {
    (void)hipStreamSynchronize(c->stream);
    return drop(rc);
  };
  elt_t* d_T[LFGPU_SC_BATCH_MAX];
  void* d_L[LFGPU_SC_BATCH_MAX];
  int rc = LFGPU_OK;
  for (size_t b = 0; b < nb; ++b) {
    lfgpu_ligero_prover* pr = out[b] = new_prover16(c, field, k, p, nullptr);
    pr->nonces.assign(h_non + b * ncols * 32, h_non + (b + 1) * ncols * 32);
    if ((rc = pr->alloc())) return fail(rc);
    d_T[b] = pr->d_T;
    d_L[b] = pr->d_layers;
  }
  void* d_non = nullptr;
  if ((rc = lf_scratch3(c, nb * ncols * 32, &d_non))) return fail(rc);
  if (hipMemcpyAsync(d_non, h_non, nb * ncols * 32, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    return fail(lf_fail(c, LFGPU_ERR_HIP, "ligero_commit_batch: nonce upload failed"));
  for (size_t b = 0; b < nb; ++b)
    if (hipMemcpy2DAsync(d_T[b], ld * 16, stage + b * img, hw * 16, hw * 16, p.nrow, hipMemcpyHostToDevice, c->stream) != hipSuccess)
      return fail(lf_fail(c, LFGPU_ERR_HIP, "ligero_commit_batch: upload failed (statement %zu)", b));
  if ((rc = ligero_extend_batch(c, pol, p, nb, d_T))) return fail(rc);
  double tv2 = 0;
  if (verbose) {
    (void)hipStreamSynchronize(c->stream);
    tv2 = lig::clock_ms();
  }
  // (ends with the one stream synchronise of the call: the uploads above are over when it returns)
  if ((rc = lfgpu_column_commit_batch(c, field, p.nrow, ld, p.dblock, ncols, nb, (const void* const*)d_T, d_non, d_L, roots_out))) return fail(rc);
  if (verbose)
    fprintf(stderr, "lfgpu ligero_commit_batch: %zu x %zu rows x %zu (block %zu, dblock %zu): host layout + draws %.2f ms | upload + RS encode %.2f | column hash + tree %.2f\n",
            nb, p.nrow, ld, p.block, p.dblock, tv1 - tv0, tv2 - tv1, lig::clock_ms() - tv2);
  return LFGPU_OK;
}

// ... over Fp256Base: the provers lfgpu_ligero_commit(field = P256) returns, their records from ONE chain of zk256.hip
extern "C" int lfgpu_ligero_commit_batch256(lfgpu_ctx* c, const lfgpu_ligero_param* pp, size_t nb, const void* const* h_W, const size_t* h_lqc,
                                            const lfgpu_rng_fn* rng, void* const* rng_user, uint8_t* roots_out, lfgpu_ligero_prover** out) {
  if (!c || !pp || !h_W || !rng || !roots_out || !out) return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit_batch256: null argument");
  if (nb == 0 || nb > LFGPU_SC_BATCH_MAX) return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit_batch256: nb = %zu, a batch holds 1..%d statements", nb, LFGPU_SC_BATCH_MAX);
  for (size_t b = 0; b < nb; ++b)
    if (!ligero_args_ok(LFGPU_FIELD_P256, 0, pp, h_W[b], h_lqc, rng[b], true))
      return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit_batch256: bad argument for statement %zu (null pointer)", b);
  for (size_t b = 0; b < nb; ++b) out[b] = nullptr;
  Lig256* L[LFGPU_SC_BATCH_MAX] = {};
  LF_TRY(lf_lig256_commit_batch(c, pp, nb, h_W, h_lqc, rng, rng_user, roots_out, L));
  for (size_t b = 0; b < nb; ++b) {
    lfgpu_ligero_prover* pr = out[b] = new lfgpu_ligero_prover();
    pr->c = c;
    pr->p = *pp;
    pr->field = LFGPU_FIELD_P256;
    pr->p256 = L[b];
  }
  return LFGPU_OK;
}

extern "C" int lfgpu_ligero_commit_sharded(lfgpu_ctx* c, int field, int k, const lfgpu_ligero_param* pp, const void* h_W, size_t subfield_boundary,
                                           const size_t* h_lqc, lfgpu_rng_fn rng, void* user, const lfgpu_comm_ops* cm, uint8_t root_out[32],
                                           lfgpu_ligero_prover** out) {
  if (!c || !pp || !root_out || !out || !comm_ok(cm) || (cm->rank == 0 && !rng) || (pp->nw && !h_W) || (pp->nq && !h_lqc))
    return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit_sharded: null argument / incomplete communicator");
  if (field != LFGPU_FIELD_GF2_128 && field != LFGPU_FIELD_FP128) return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit_sharded: field");
  const lfgpu_ligero_param& p = *pp;
  if (p.ildt != 0 || p.idot != 1 || p.iquad != 2 || p.iw != 3) return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit_sharded: row order");
  LF_HIP(c, hipSetDevice(c->device));
  const L16 pol = policy16(c, field, k);
  if (field == LFGPU_FIELD_GF2_128 && !pol.g) return lf_fail(c, LFGPU_ERR_ARG, "ligero_commit_sharded: k");
  const double t0 = lig::clock_ms();
  std::unique_ptr<lfgpu_ligero_prover> pr(new_prover16(c, field, k, p, cm));
  // host layout of this rank's slab from the one random stream; then the slab is encoded (rows are independent) and the columns go
  // through all_to_all, local leaves, all_gather of the digests and the tree on every rank
  std::vector<elt_t> H(std::max<size_t>(pr->row_hi - pr->row_lo, 1) * p.dblock);
  LF_SCRUB_ON_EXIT(H);
  char err[256] = {0};
  const int rc = layout_sharded_host(pol, p, h_W, subfield_boundary, h_lqc, rng, user, cm, c->rng_exact != 0, pr->row_lo, pr->row_hi, H.data(), pr->nonces.data(), err);
  if (rc) return lf_fail(c, rc, "%s", err);
  LF_TRY(lig::commit_rows(pr.get(), pol, H.data(), t0, root_out));
  *out = pr.release();
  return LFGPU_OK;
}

extern "C" int lfgpu_ligero_inner_product_rows(lfgpu_ctx* c, int field, size_t w, size_t r, size_t ld, size_t nrows, const void* d_dense,
                                               size_t ndense, const uint64_t scale[2], const uint64_t* h_idx, const void* h_val,
                                               size_t nsparse, void* d_rows) {
  if (!c || !d_rows || w == 0 || r + w > ld || (ndense && (!d_dense || !scale)) || (nsparse && (!h_idx || !h_val)) || ndense > nrows * w)
    return lf_fail(c, LFGPU_ERR_ARG, "ligero_inner_product_rows: bad argument");
  if (field != LFGPU_FIELD_GF2_128 && field != LFGPU_FIELD_FP128) return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "ligero_inner_product_rows: field");
  LF_HIP(c, hipSetDevice(c->device));
  const elt_t sc = scale ? elt_t{scale[0], scale[1]} : elt_t{0, 0};
  return lig::a_rows(c, L16{{field, 0, nullptr}}, w, r, ld, nrows, (const elt_t*)d_dense, ndense, sc, h_idx, (const elt_t*)h_val, nsparse, (elt_t*)d_rows);
}

extern "C" int lfgpu_ligero_low_degree_proof(lfgpu_ligero_prover* pr, const void* h_u, void* h_y) {
  if (!pr || !h_u || !h_y) return LFGPU_ERR_ARG;
  LF_HIP(pr->c, hipSetDevice(pr->c->device));
  if (pr->p256) return lf_lig256_low_degree(pr->p256, h_u, h_y);
  return lig::low_degree(pr, policy16(pr), (const elt_t*)h_u, (elt_t*)h_y);
}

extern "C" int lfgpu_ligero_dot_proof(lfgpu_ligero_prover* pr, const void* h_A, void* h_y) {
  if (!pr || !h_A || !h_y) return LFGPU_ERR_ARG;
  lfgpu_ctx* c = pr->c;
  const lfgpu_ligero_param& p = pr->p;
  LF_HIP(c, hipSetDevice(c->device));
  if (pr->p256) return lf_lig256_dot_dense(pr->p256, h_A, h_y);
  const size_t lda = p.dblock;
  void* sc = nullptr;
  LF_TRY(lf_scratch3(c, (p.nwqrow * p.w + p.nwqrow * lda + 2 * p.dblock) * 16 + 64, &sc));
  elt_t* dA = (elt_t*)sc;
  elt_t* dAext = dA + p.nwqrow * p.w;
  elt_t* dy = dAext + p.nwqrow * lda;
  LF_HIP(c, hipMemcpyAsync(dA, h_A, p.nwqrow * p.w * 16, hipMemcpyHostToDevice, c->stream));
  LF_HIP(c, hipMemsetAsync(dAext, 0, p.nwqrow * lda * 16, c->stream));
  hipLaunchKernelGGL(layout_aext_kernel, dim3((u32)((p.block + 255) / 256), (u32)p.nwqrow), dim3(256), 0, c->stream,
                     (u32)p.r, (u32)p.w, lda, (const elt_t*)dA, dAext);
  return lig::dot_finish(pr, policy16(pr), dAext, dy, (elt_t*)h_y);
}

extern "C" int lfgpu_ligero_dot_proof_sparse(lfgpu_ligero_prover* pr, const void* d_dense, size_t ndense, const uint64_t scale[2],
                                             const uint64_t* h_idx, const void* h_val, size_t nsparse, void* h_y) {
  if (!pr || !h_y) return LFGPU_ERR_ARG;
  if (pr->p256) return lf_fail(pr->c, LFGPU_ERR_ARG, "ligero_dot_proof_sparse: 16-byte fields only (an Fp256Base prover takes lfgpu_ligero_dot_proof or lfgpu_ligero_prove256)");
  if (ndense && !scale) return lf_fail(pr->c, LFGPU_ERR_ARG, "ligero_dot_proof_sparse: a dense block needs its scale");
  LF_HIP(pr->c, hipSetDevice(pr->c->device));
  const elt_t sc = scale ? elt_t{scale[0], scale[1]} : elt_t{0, 0};
  return lig::dot(pr, policy16(pr), (const elt_t*)d_dense, ndense, sc, h_idx, (const elt_t*)h_val, nsparse, (elt_t*)h_y);
}

// ---- below the C ABI, for lfgpu_ligero_prove / lfgpu_ligero_verify (zk.hip; declared in zkint.h)
int lf_ligero_a_rows_terms(lfgpu_ctx* c, int field, const lfgpu_ligero_param* p, size_t ld, const LfLigeroTerms* t, void* d_rows) {
  return L16{{field, 0, nullptr}}.a_rows_terms(c, *p, ld, *t, (elt_t*)d_rows);
}
int lf_ligero_dot_terms(lfgpu_ligero_prover* pr, const LfLigeroTerms* t, void* h_y) {
  LF_HIP(pr->c, hipSetDevice(pr->c->device));
  return lig::dot_terms(pr, policy16(pr), *t, (elt_t*)h_y);
}
void lf_ligero_prover_view(lfgpu_ligero_prover* pr, LfLigeroView* v) {
  v->c = pr->c;
  v->field = pr->field;
  v->k = pr->k;
  v->p = pr->p;
  v->whole = !pr->sharded && pr->owns && pr->row_lo == 0 && pr->row_hi == pr->p.nrow;
  v->wire = &pr->wire;
  v->wire_held = &pr->wire_held;
  v->lig256 = pr->p256;
}

extern "C" int lfgpu_ligero_quadratic_proof(lfgpu_ligero_prover* pr, const void* h_u_quad, void* h_y0, void* h_y2) {
  if (!pr || !h_y0 || !h_y2 || (pr->p.nqtriples && !h_u_quad)) return LFGPU_ERR_ARG;
  LF_HIP(pr->c, hipSetDevice(pr->c->device));
  if (pr->p256) return lf_lig256_quadratic(pr->p256, h_u_quad, h_y0, h_y2);
  return lig::quadratic(pr, policy16(pr), (const elt_t*)h_u_quad, (elt_t*)h_y0, (elt_t*)h_y2);
}

// a prover over rows [row_lo, row_hi) that the caller has laid out and encoded (lfgpu_ligero_encode_rows) in d_slab;
// d_layers / h_nonces: the Merkle heap and nonces of the whole commitment (for lfgpu_ligero_open), may be null
extern "C" int lfgpu_ligero_prover_from_slab(lfgpu_ctx* c, int field, int k, const lfgpu_ligero_param* pp, size_t row_lo, size_t row_hi,
                                             void* d_slab, void* d_layers, const uint8_t* h_nonces, lfgpu_ligero_prover** out) {
  if (!c || !pp || !out || row_lo > row_hi || row_hi > pp->nrow || (row_hi > row_lo && !d_slab))
    return lf_fail(c, LFGPU_ERR_ARG, "ligero_prover_from_slab: bad argument");
  if (field != LFGPU_FIELD_GF2_128 && field != LFGPU_FIELD_FP128) return lf_fail(c, LFGPU_ERR_ARG, "ligero_prover_from_slab: field");
  lfgpu_ligero_prover* pr = new_prover16(c, field, k, *pp, nullptr);
  pr->borrow(row_lo, row_hi, (elt_t*)d_slab, (uint8_t*)d_layers, h_nonces);
  *out = pr;
  return LFGPU_OK;
}

extern "C" int lfgpu_ligero_open(lfgpu_ligero_prover* pr, const size_t* idx, void* h_req, uint8_t* h_nonces,
                                 uint8_t* h_path, size_t path_cap, size_t* npath) {
  if (!pr || !idx || !h_req || !h_nonces || !npath) return LFGPU_ERR_ARG;
  if (pr->p256) {
    LF_HIP(pr->c, hipSetDevice(pr->c->device));
    return lf_lig256_open(pr->p256, idx, h_req, h_nonces, h_path, path_cap, npath);
  }
  return lig::open(pr, policy16(pr), idx, (elt_t*)h_req, h_nonces, h_path, path_cap, npath);
}

// ------------------------------------------------------------------ LigeroProver::prove for nb committed provers of one shape
// (lig::prove_batch / lig::open_batch, ligero_slab.h, over L16)
extern "C" int lfgpu_ligero_prove_batch(lfgpu_ctx* c, lfgpu_ligero_prover* const* pr, size_t nb, const void* h_u_ldt, const void* const* d_dense,
                                        size_t ndense, const uint64_t* scale, const uint64_t* const* h_idx, const void* const* h_val,
                                        const size_t* nsparse, const void* h_u_quad, void* h_y_ldt, void* h_y_dot, void* h_y_q0, void* h_y_q2) {
  if (!c || !pr || !nsparse || !h_y_ldt || !h_y_dot || !h_y_q0 || !h_y_q2) return lf_fail(c, LFGPU_ERR_ARG, "ligero_prove_batch: null argument");
  return lig::prove_batch<L16>(c, "ligero_prove_batch", pr, nb, h_u_ldt, d_dense, ndense, scale, h_idx, h_val, nsparse, h_u_quad, h_y_ldt, h_y_dot, h_y_q0, h_y_q2);
}
extern "C" int lfgpu_ligero_open_batch(lfgpu_ctx* c, lfgpu_ligero_prover* const* pr, size_t nb, const size_t* idx, void* h_req, uint8_t* h_nonces,
                                       uint8_t* h_path, size_t path_cap, size_t* npath) {
  if (!c || !pr || !idx || !h_req || !h_nonces || !npath) return lf_fail(c, LFGPU_ERR_ARG, "ligero_open_batch: null argument");
  return lig::open_batch<L16>(c, "ligero_open_batch", pr, nb, idx, h_req, h_nonces, h_path, path_cap, npath);
}
