// ligero_slab.h -- the prover that holds a slab of a Ligero tableau: its record, its commit side and its prove-side calls, written
// once over a width policy L.
//
// ligero.hip (GF(2^128) and Fp128, 16-byte elements) and zk256.hip (Fp256Base, 32-byte elements) each supply a policy and
// instantiate what is here.  Reference: LigeroProver::commit / low_degree_proof / dot_proof / quadratic_proof / compute_req
// (lib/ligero/ligero_prover.h:58-79,281-351), inner_product_vector + layout_Aext (lib/ligero/ligero_param.h:382-430),
// MerkleCommitment (lib/merkle/merkle_commitment.h:50-73).
//
// A policy is a plain struct with no virtual calls.  It derives from its host policy (ligero_layout.h: the element
// type E, the field id, host add / is_zero, the RandomEngine draws) and adds the device steps the bodies call; each step uploads
// its own host vectors the way its width always has (and synchronises where it always has), so nothing below tests which width
// it serves:
//   rows_axpy      y[j] += sum_i u[i] T[i][j], u on the host
//   rows_vaxpy     y[j] = T0[j] + sum_i A[i][j] T[i][j]
//   quad_combo     y[j] = Tq[j] + sum_i u[i] (Z_i[j] - X_i[j] Y_i[j])
//   a_rows_clear / a_rows_dense / a_rows_sparse   the pieces of a_rows below; the sparse lists are on the host
//   a_rows_terms   rows += inner_product_vector of a term list in any order, duplicates allowed
//   gather_columns req[i][j] = T[i][col0 + idx[j]], idx on the host
//   rs_rows        nrow rows of n values extended to m, in place
//   rs_rows_mixed  a slab's three row groups in one launch where the width has such a kernel, else LFGPU_ERR_UNSUPPORTED
//   column_leaves  the leaf digests of ncols columns
// and for the batched prove and open of nb whole-tableau provers of one shape (prove_batch / open_batch; every vector is on the
// device, cb statements of a chain at one stride each, tableaux and dense blocks as LfBatchPtrs; these only enqueue):
//   batch_ok             what the width asks of the provers beyond batch_core; yields the policy
//   batch_rs_cap         the most statements the encoder of a chain's A rows takes
//   a_rows_dense_batch / a_rows_sparse_batch   a_rows of every statement, the sparse lists packed behind one another
//   rs_rows_batch        the A rows of every statement extended in place
//   rows_combo_batch     y_b = T_b[ildt] + sum_i u_b[i] T_b[iw + i] over block columns | T_b[idot] + sum_i A_b[i] T_b[iw + i] over dblock
//   quad_combo_batch     quad_combo of every statement
//   gather_columns_batch gather_columns of every statement, idx [cb][nreq]
// The commit side: Slab::init / alloc build the record, extend_slab Reed-Solomon-encodes a fresh slab, commit_rows uploads a
// slab's host image, encodes it and commits the columns (one GPU, or the sharded exchange).  What stays in the two files: the
// entry points with their null-argument checks and their own layout call (ligero_layout.h; the sharded record / replay of the
// engine), each width's own demands on the provers of a batch, and every kernel.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "ctx.h"
#include "ligero_layout.h"

// Everything below has internal linkage (as in zk_proto.h): each file that includes this header wants its own copy.
namespace lig {
namespace {
template <class E>
struct Slab {
  lfgpu_ctx* c = nullptr;
  lfgpu_ligero_param p{};
  E* d_T = nullptr;             // [row_hi - row_lo][block_enc]
  uint8_t* d_layers = nullptr;  // [2*block_ext][32]
  size_t T_bytes = 0, L_bytes = 0;
  std::vector<uint8_t> nonces;  // block_ext * 32 (host copy for open)
  // rows [row_lo, row_hi) of the tableau live in d_T (a slab of a multi-GPU commit; [0, nrow) on one GPU).  The prove
  // functions then return this slab's PARTIAL sums (rows it does not hold contribute zero); the caller folds the ranks.
  size_t row_lo = 0, row_hi = 0;
  bool owns = true;  // d_T / d_layers go back to the pool with the prover
  // a prover of a sharded commit: the prove functions fold the ranks' partial results through these hooks
  bool sharded = false;
  lfgpu_comm_ops comm{};
  std::vector<std::pair<size_t, size_t>> spans;  // row slab of every rank
  bool has(size_t i) const { return i >= row_lo && i < row_hi; }
  E* row(size_t i) const { return d_T + (i - row_lo) * p.block_enc; }
  Slab() = default;
  // the record of a commit: parameters, room for the nonces and the slab -- [0, nrow), or with a communicator this rank's rows
  // of lfgpu_ligero_row_shard next to every rank's span
  void init(lfgpu_ctx* ctx, const lfgpu_ligero_param& param, const lfgpu_comm_ops* cm) {
    c = ctx;
    p = param;
    nonces.resize(32 * p.block_ext);
    row_lo = 0;
    row_hi = p.nrow;
    if (!cm) return;
    sharded = true;
    comm = *cm;
    spans.resize(cm->world);
    for (int q = 0; q < cm->world; ++q) (void)lfgpu_ligero_row_shard(&p, q, cm->world, &spans[q].first, &spans[q].second);
    row_lo = spans[cm->rank].first;
    row_hi = spans[cm->rank].second;
  }
  // tableau and Merkle heap: buffers of an earlier prover with the same shape where there is one (the context's pool)
  int alloc() {
    T_bytes = std::max<size_t>(row_hi - row_lo, 1) * p.block_enc * sizeof(E);
    L_bytes = 2 * p.block_ext * 32;
    if (lf_pool_get(c, T_bytes, (void**)&d_T) != LFGPU_OK || lf_pool_get(c, L_bytes, (void**)&d_layers) != LFGPU_OK)
      return lf_fail(c, LFGPU_ERR_NOMEM, "ligero commit: tableau / Merkle heap alloc (rows [%zu, %zu))", row_lo, row_hi);
    return LFGPU_OK;
  }
  // ... or rows [lo, hi) that the caller has encoded in a buffer of its own; layers / h_nonces: the Merkle heap and the nonces of
  // the whole commitment, may be null (then `open` answers that the prover holds no commitment)
  void borrow(size_t lo, size_t hi, E* T, uint8_t* layers, const uint8_t* h_nonces) {
    row_lo = lo;
    row_hi = hi;
    d_T = T;
    d_layers = layers;
    owns = false;
    if (h_nonces) nonces.assign(h_nonces, h_nonces + 32 * p.block_ext);
    else nonces.clear();
  }
  Slab(const Slab&) = delete;
  Slab& operator=(const Slab&) = delete;
  ~Slab() {
    // keep the buffers for the next commit of the same shape (the context's pool: a hipFree per proof would wait for every
    // stream of the device); the stream is in order, so work still queued on them finishes before anything a later commit enqueues
    auto stash = [&](void* d, size_t bytes) {
      if (!d) return;
      // the tableau holds the witness, the pads and the blinding rows: scrub it before it outlives its prover (enqueued on the
      // stream, in order behind the prover's last kernels)
      if (bytes) (void)hipMemsetAsync(d, 0, bytes, c ? c->stream : nullptr);
      if (c && bytes) lf_pool_put(c, d, bytes);
      else (void)hipFree(d);
    };
    if (!owns) return;
    stash(d_T, T_bytes);
    stash(d_layers, L_bytes);
  }
};

inline double clock_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The context's pinned staging of a batched commit (ctx.h: cb_stage_h), at least `used` bytes: kept from call to call, replaced by
// a larger one when a call needs more.  The uploads of the previous call are over (every call ends with a stream synchronise), so
// the memory may be rewritten at once.  The caller scrubs what it wrote before it returns (CbScrub).
inline int cb_stage(lfgpu_ctx* c, const char* who, size_t used, uint8_t** out) {
  if (c->cb_stage_bytes < used) {
    if (c->cb_stage_h) (void)hipHostFree(c->cb_stage_h);  // (scrubbed after the call that filled it)
    c->cb_stage_h = nullptr;
    c->cb_stage_bytes = 0;
    if (hipHostMalloc(&c->cb_stage_h, used, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      c->cb_stage_h = nullptr;
      return lf_fail(c, LFGPU_ERR_NOMEM, "%s: %zu bytes of pinned staging", who, used);
    }
    c->cb_stage_bytes = used;
  }
  *out = (uint8_t*)c->cb_stage_h;
  return LFGPU_OK;
}
struct CbScrub {  // the images hold the witnesses, the pads and the blinding rows
  uint8_t* p;
  size_t n;
  ~CbScrub() { explicit_bzero(p, n); }
};

inline void shard_split(size_t n, int rank, int world, size_t* start, size_t* count) {  // contiguous, sizes differ by at most 1
  const size_t base = n / (size_t)world, rem = n % (size_t)world, r = (size_t)rank;
  *start = r * base + std::min(r, rem);
  *count = base + (r < rem ? 1 : 0);
}

// field sum over the ranks of a host vector every rank holds a partial of (RCCL has no XOR / mod-p reduction: all_gather + fold);
// nothing to do for a prover that is not sharded
template <class L>
int comm_fold(const Slab<typename L::E>* pr, const L& pol, typename L::E* y, size_t n) {
  using E = typename L::E;
  const lfgpu_comm_ops& cm = pr->comm;
  if (!pr->sharded || cm.world == 1) return LFGPU_OK;
  std::vector<E> all((size_t)cm.world * n);
  LF_SCRUB_ON_EXIT(all);  // the ranks' partial sums are not part of the proof; only their fold is
  if (cm.all_gather(cm.user, y, all.data(), n * sizeof(E), 0, nullptr)) return lf_fail(pr->c, LFGPU_ERR_HIP, "ligero (sharded): all_gather hook failed");
  for (size_t j = 0; j < n; ++j) y[j] = all[j];
  for (int q = 1; q < cm.world; ++q)
    for (size_t j = 0; j < n; ++j) y[j] = pol.add(y[j], all[(size_t)q * n + j]);
  return LFGPU_OK;
}

// witness / quadratic rows [a_lo, a_hi) (indices relative to iw) that this prover's slab holds
template <class E>
void owned_wq_rows(const Slab<E>* pr, size_t* a_lo, size_t* a_hi) {
  const lfgpu_ligero_param& p = pr->p;
  const size_t lo = std::min(std::max(pr->row_lo, p.iw), p.iw + p.nwqrow), hi = std::min(std::max(pr->row_hi, p.iw), p.iw + p.nwqrow);
  *a_lo = lo - p.iw;
  *a_hi = std::max(hi, lo) - p.iw;
}

// low_degree_proof (:281-291)
template <class L>
int low_degree(Slab<typename L::E>* pr, const L& pol, const typename L::E* u, typename L::E* y) {
  using E = typename L::E;
  lfgpu_ctx* c = pr->c;
  const lfgpu_ligero_param& p = pr->p;
  void* dy = nullptr;
  LF_TRY(lf_scratch3(c, p.block * sizeof(E), &dy));
  if (pr->has(p.ildt))
    LF_HIP(c, hipMemcpyAsync(dy, pr->row(p.ildt), p.block * sizeof(E), hipMemcpyDeviceToDevice, c->stream));
  else
    LF_HIP(c, hipMemsetAsync(dy, 0, p.block * sizeof(E), c->stream));
  size_t a_lo, a_hi;
  owned_wq_rows(pr, &a_lo, &a_hi);
  if (a_hi > a_lo) LF_TRY(pol.rows_axpy(c, a_hi - a_lo, p.block, (E*)dy, u + a_lo, pr->row(p.iw + a_lo), p.block_enc));
  LF_TRY(lfgpu_memcpy_d2h(c, y, dy, p.block * sizeof(E)));
  return comm_fold(pr, pol, y, p.block);
}

// ---- the inner-product matrix built on the device (inner_product_vector + layout_Aext, ligero_param.h:382-430)
// rows[i][r + j] = scale * dense[i*w + j] over the first ndense flat positions (the private-input block of the last
// constraint), then rows[pos(idx)] += val for the caller's sparse terms.  The sparse kernels read, add and write without
// atomics, so the indices must be strictly increasing (duplicates already folded by the caller) and in range.
template <class L>
int a_rows(lfgpu_ctx* c, const L& pol, size_t w, size_t r, size_t ld, size_t nrows, const typename L::E* d_dense, size_t ndense,
           const typename L::E& scale, const uint64_t* h_idx, const typename L::E* h_val, size_t nsparse, typename L::E* d_rows) {
  if (ndense > nrows * w || (ndense && !d_dense) || (nsparse && (!h_idx || !h_val))) return lf_fail(c, LFGPU_ERR_ARG, "ligero inner-product rows: bad argument");
  for (size_t t = 0; t < nsparse; ++t) {
    if (h_idx[t] >= nrows * w) return lf_fail(c, LFGPU_ERR_ARG, "ligero inner-product rows: sparse index out of range");
    if (t && h_idx[t] <= h_idx[t - 1]) return lf_fail(c, LFGPU_ERR_ARG, "ligero inner-product rows: sparse indices must be strictly increasing");
  }
  LF_TRY(pol.a_rows_clear(c, d_rows, ld, r + w, nrows));
  if (ndense) LF_TRY(pol.a_rows_dense(c, r, w, ld, scale, d_dense, ndense, d_rows));
  if (nsparse) LF_TRY(pol.a_rows_sparse(c, r, w, ld, h_idx, h_val, nsparse, nrows * w, d_rows));
  return LFGPU_OK;
}

// dot_proof (:293-309) once the rows [0^r | A_i | 0...] stand in dAext (lda = dblock; all nwqrow rows, of which the slab's are
// used; a spare row of dblock elements behind dy): extend, combine, read back
template <class L>
int dot_finish(Slab<typename L::E>* pr, const L& pol, typename L::E* dAext, typename L::E* dy, typename L::E* y) {
  using E = typename L::E;
  lfgpu_ctx* c = pr->c;
  const lfgpu_ligero_param& p = pr->p;
  const size_t lda = p.dblock;
  size_t a_lo, a_hi;
  owned_wq_rows(pr, &a_lo, &a_hi);
  const E* T0 = nullptr;
  if (pr->has(p.idot)) {
    T0 = pr->row(p.idot);
  } else {  // a zero row behind dy
    LF_HIP(c, hipMemsetAsync(dy + p.dblock, 0, p.dblock * sizeof(E), c->stream));
    T0 = dy + p.dblock;
  }
  if (a_hi > a_lo) LF_TRY(pol.rs_rows(c, a_hi - a_lo, p.block, p.dblock, dAext + a_lo * lda, lda));
  LF_TRY(pol.rows_vaxpy(c, a_hi - a_lo, p.dblock, T0, dAext + a_lo * lda, lda, a_hi > a_lo ? pr->row(p.iw + a_lo) : pr->d_T, p.block_enc, dy));
  LF_TRY(lfgpu_memcpy_d2h(c, y, dy, p.dblock * sizeof(E)));
  return comm_fold(pr, pol, y, p.dblock);
}
// ... with A given as inner_product_vector builds it: scale * dense[0..ndense) over the first flat positions plus the sparse terms
template <class L>
int dot(Slab<typename L::E>* pr, const L& pol, const typename L::E* d_dense, size_t ndense, const typename L::E& scale, const uint64_t* h_idx,
        const typename L::E* h_val, size_t nsparse, typename L::E* y) {
  using E = typename L::E;
  lfgpu_ctx* c = pr->c;
  const lfgpu_ligero_param& p = pr->p;
  const size_t lda = p.dblock, bytes = (p.nwqrow * lda + 2 * p.dblock) * sizeof(E);
  void* sc = nullptr;
  LF_TRY(lf_scratch3(c, bytes + 64, &sc));
  if (d_dense && ndense) {  // the dense block must not live in the scratch this call is about to overwrite
    const uint8_t* lo = (const uint8_t*)sc;
    const uint8_t* d = (const uint8_t*)d_dense;
    if (d + ndense * sizeof(E) > lo && d < lo + bytes) return lf_fail(c, LFGPU_ERR_ARG, "ligero dot proof: dense block aliases scratch");
  }
  E* dAext = (E*)sc;
  LF_HIP(c, hipMemsetAsync(dAext, 0, p.nwqrow * lda * sizeof(E), c->stream));
  LF_TRY(a_rows(c, pol, p.w, p.r, lda, p.nwqrow, d_dense, ndense, scale, h_idx, h_val, nsparse, dAext));
  return dot_finish(pr, pol, dAext, dAext + p.nwqrow * lda, y);
}

// ... with A accumulated on the device from a term list in any order (pol.a_rows_terms)
template <class L, class Terms>
int dot_terms(Slab<typename L::E>* pr, const L& pol, const Terms& t, typename L::E* y) {
  using E = typename L::E;
  lfgpu_ctx* c = pr->c;
  const lfgpu_ligero_param& p = pr->p;
  const size_t lda = p.dblock, bytes = (p.nwqrow * lda + 2 * p.dblock) * sizeof(E);
  void* sc = nullptr;
  LF_TRY(lf_scratch3(c, bytes + 64, &sc));
  E* dAext = (E*)sc;
  LF_HIP(c, hipMemsetAsync(dAext, 0, p.nwqrow * lda * sizeof(E), c->stream));
  LF_TRY(pol.a_rows_terms(c, p, lda, t, dAext));
  return dot_finish(pr, pol, dAext, dAext + p.nwqrow * lda, y);
}

// quadratic_proof (:311-344)
template <class L>
int quadratic(Slab<typename L::E>* pr, const L& pol, const typename L::E* u, typename L::E* y0, typename L::E* y2) {
  using E = typename L::E;
  lfgpu_ctx* c = pr->c;
  const lfgpu_ligero_param& p = pr->p;
  // a triple (x_i, y_i, z_i) is multiplied element-wise, so a slab must hold all quadratic rows or none of them
  const size_t q_lo = p.iq, q_hi = p.iq + 3 * p.nqtriples;
  const bool all_q = p.nqtriples == 0 || (pr->row_lo <= q_lo && q_hi <= pr->row_hi);
  const bool no_q = pr->row_hi <= q_lo || pr->row_lo >= q_hi;
  if (!all_q && !no_q) return lf_fail(c, LFGPU_ERR_ARG, "quadratic_proof: the slab splits the quadratic rows (shard so that one rank holds [iq, nrow))");
  const size_t nt = all_q ? p.nqtriples : 0;
  void* sc = nullptr;
  LF_TRY(lf_scratch3(c, (p.nqtriples + 1 + 2 * p.dblock) * sizeof(E) + 64, &sc));
  E* du = (E*)sc;
  E* dy = du + p.nqtriples + 1;
  E* dz = dy + p.dblock;
  if (nt) LF_HIP(c, hipMemcpyAsync(du, u, p.nqtriples * sizeof(E), hipMemcpyHostToDevice, c->stream));
  const size_t ld = p.block_enc;
  const E* Tq = nullptr;
  if (pr->has(p.iquad)) {
    Tq = pr->row(p.iquad);
  } else {
    LF_HIP(c, hipMemsetAsync(dz, 0, p.dblock * sizeof(E), c->stream));
    Tq = dz;
  }
  const E* X = nt ? pr->row(p.iq) : pr->d_T;
  const E* Y = X + p.nqtriples * ld;
  const E* Z = Y + p.nqtriples * ld;
  LF_TRY(pol.quad_combo(c, nt, p.dblock, Tq, du, X, Y, Z, ld, dy));
  std::vector<E> y(p.dblock);
  LF_TRY(lfgpu_memcpy_d2h(c, y.data(), dy, p.dblock * sizeof(E)));
  LF_TRY(comm_fold(pr, pol, y.data(), p.dblock));
  if (pr->sharded || (pr->row_lo == 0 && pr->row_hi == p.nrow))  // sanity check of the reference (:335-337); a bare slab's partial sums are checked by its caller after the fold
    for (size_t j = 0; j < p.w; ++j)
      if (!pol.is_zero(y[p.r + j])) return lf_fail(c, LFGPU_ERR_ASSERT, "quadratic_proof: W part is nonzero");
  memcpy(y0, y.data(), p.r * sizeof(E));
  memcpy(y2, y.data() + p.block, (p.dblock - p.block) * sizeof(E));
  return LFGPU_OK;
}

// compute_req + MerkleCommitment::open
template <class L>
int open(Slab<typename L::E>* pr, const L& pol, const size_t* idx, typename L::E* h_req, uint8_t* h_nonces, uint8_t* h_path, size_t path_cap, size_t* npath) {
  using E = typename L::E;
  lfgpu_ctx* c = pr->c;
  const lfgpu_ligero_param& p = pr->p;
  for (size_t i = 0; i < p.nreq; ++i)
    if (idx[i] >= p.block_ext) return lf_fail(c, LFGPU_ERR_ARG, "ligero_open: index out of range");
  if (pr->nonces.size() != 32 * p.block_ext || !pr->d_layers) return lf_fail(c, LFGPU_ERR_ARG, "ligero_open: this prover holds no commitment");
  // a slab returns its own rows of req ((row_hi - row_lo) x nreq, in row order); a sharded prover gathers every rank's rows
  const size_t nr = pr->row_hi - pr->row_lo;
  std::vector<uint8_t> mine;  // padded to the largest slab for the all_gather
  size_t maxr = nr;
  if (pr->sharded) {
    for (const auto& sp : pr->spans) maxr = std::max(maxr, sp.second - sp.first);
    mine.assign(maxr * p.nreq * sizeof(E), 0);
  }
  void* h_dst = pr->sharded ? (void*)mine.data() : (void*)h_req;
  if (nr) {
    void* dreq = nullptr;
    LF_TRY(lf_scratch3(c, nr * p.nreq * sizeof(E), &dreq));
    LF_TRY(pol.gather_columns(c, nr, p.block_enc, p.dblock, pr->d_T, idx, p.nreq, (E*)dreq));
    LF_TRY(lfgpu_memcpy_d2h(c, h_dst, dreq, nr * p.nreq * sizeof(E)));
  }
  if (pr->sharded) {
    const lfgpu_comm_ops& cm = pr->comm;
    std::vector<uint8_t> all((size_t)cm.world * mine.size());
    if (cm.all_gather(cm.user, mine.data(), all.data(), mine.size(), 0, nullptr)) return lf_fail(c, LFGPU_ERR_HIP, "ligero_open (sharded): all_gather hook failed");
    for (int q = 0; q < cm.world; ++q)
      memcpy((uint8_t*)h_req + pr->spans[q].first * p.nreq * sizeof(E), all.data() + (size_t)q * mine.size(),
             (pr->spans[q].second - pr->spans[q].first) * p.nreq * sizeof(E));
  }
  for (size_t i = 0; i < p.nreq; ++i) memcpy(h_nonces + 32 * i, &pr->nonces[32 * idx[i]], 32);
  return lfgpu_merkle_open(c, p.block_ext, pr->d_layers, idx, p.nreq, h_path, path_cap, npath);
}

// The column commitment of a sharded prover whose slab stands encoded in d_T (spans, row_lo / row_hi, nonces and d_layers set).
// A leaf hashes ALL rows of one column: one all_to_all re-partitions the encoded columns [dblock, block_enc) so that this rank
// owns columns [mc0, mc0 + mcn) of every row; then local leaves, an all_gather of the digests and the tree on every rank
// (lfgpu_merkle_build_tree ends with a stream synchronise).  Byte-oriented: only the element size and the leaf hash are the policy's.
// t_begin: clock_ms() when the caller began to upload and encode the slab, for the LFGPU_VERBOSE phase line.
template <class L>
int column_commit_sharded(Slab<typename L::E>* pr, const L& pol, double t_begin, uint8_t root_out[32]) {
  constexpr size_t esz = sizeof(typename L::E);
  lfgpu_ctx* c = pr->c;
  const lfgpu_ligero_param& p = pr->p;
  const lfgpu_comm_ops* cm = &pr->comm;
  const int world = cm->world, rank = cm->rank;
  const size_t nr = pr->row_hi - pr->row_lo, ld = p.block_enc, ncols = p.block_ext;
  static const bool verbose = getenv("LFGPU_VERBOSE") != nullptr;
  double tv2 = t_begin;
  void* d_send = nullptr;
  void* d_cols = nullptr;
  size_t send_bytes_tot = 0, cols_bytes = 0;
  // the exchange buffers hold encoded rows of the tableau (witness, pads, blinding rows): scrubbed like the tableau itself
  // (~Slab) before they go back to the pool, in stream order behind their last use
  auto retire = [&](void*& d, size_t bytes) {
    if (!d) return;
    (void)hipMemsetAsync(d, 0, bytes, c->stream);
    lf_pool_put(c, d, bytes);
    d = nullptr;
  };
  auto done = [&](int rc) {
    retire(d_send, send_bytes_tot);
    retire(d_cols, cols_bytes);
    return rc;
  };
  // Send block for rank q: my rows x its columns, contiguous.
  std::vector<size_t> soff(world), sbytes(world), roff(world), rbytes(world);
  size_t mc0 = 0, mcn = 0;
  shard_split(ncols, rank, world, &mc0, &mcn);
  for (int q = 0; q < world; ++q) {
    size_t c0, cn;
    shard_split(ncols, q, world, &c0, &cn);
    soff[q] = send_bytes_tot;
    sbytes[q] = nr * cn * esz;
    send_bytes_tot += sbytes[q];
    roff[q] = pr->spans[q].first * mcn * esz;  // slabs are contiguous and ascending: the received blocks ARE the column matrix
    rbytes[q] = (pr->spans[q].second - pr->spans[q].first) * mcn * esz;
  }
  cols_bytes = std::max<size_t>(p.nrow * mcn * esz, esz);
  send_bytes_tot = std::max<size_t>(send_bytes_tot, esz);
  if (lf_pool_get(c, send_bytes_tot, &d_send) != LFGPU_OK || lf_pool_get(c, cols_bytes, &d_cols) != LFGPU_OK)
    return done(lf_fail(c, LFGPU_ERR_NOMEM, "ligero (sharded): exchange buffers"));
  for (int q = 0; q < world && nr; ++q) {
    size_t c0, cn;
    shard_split(ncols, q, world, &c0, &cn);
    if (cn && hipMemcpy2DAsync((uint8_t*)d_send + soff[q], cn * esz, pr->d_T + p.dblock + c0, ld * esz, cn * esz, nr, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
      return done(lf_fail(c, LFGPU_ERR_HIP, "ligero (sharded): pack"));
  }
  if (verbose) {
    (void)hipStreamSynchronize(c->stream);
    tv2 = clock_ms();
  }
  if (cm->all_to_all(cm->user, d_send, soff.data(), sbytes.data(), d_cols, roff.data(), rbytes.data(), 1, c->stream))
    return done(lf_fail(c, LFGPU_ERR_HIP, "ligero (sharded): all_to_all hook failed"));
  const double tv3 = clock_ms();
  // local leaves of my columns, all_gather of the digests (ragged: padded to the largest share), the tree on every rank
  size_t maxn = 0, dummy = 0;
  shard_split(ncols, 0, world, &dummy, &maxn);
  void* d_non = nullptr;
  int rc = lf_scratch3(c, ncols * 32 + (size_t)(world + 1) * maxn * 32 + 64, &d_non);
  if (rc) return done(rc);
  uint8_t* d_mine = (uint8_t*)d_non + ncols * 32;
  uint8_t* d_all = d_mine + maxn * 32;
  if (hipMemcpyAsync(d_non, pr->nonces.data(), ncols * 32, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemsetAsync(d_mine, 0, maxn * 32, c->stream) != hipSuccess)
    return done(lf_fail(c, LFGPU_ERR_HIP, "ligero (sharded): nonce upload"));
  if (mcn && (rc = pol.column_leaves(c, p.nrow, mcn, 0, mcn, d_cols, (const uint8_t*)d_non + mc0 * 32, d_mine))) return done(rc);
  if (cm->all_gather(cm->user, d_mine, d_all, maxn * 32, 1, c->stream)) return done(lf_fail(c, LFGPU_ERR_HIP, "ligero (sharded): all_gather hook failed"));
  if (hipMemsetAsync(pr->d_layers, 0, ncols * 32, c->stream) != hipSuccess) return done(lf_fail(c, LFGPU_ERR_HIP, "ligero (sharded): layers"));
  for (int q = 0; q < world; ++q) {
    size_t c0, cn;
    shard_split(ncols, q, world, &c0, &cn);
    if (cn && hipMemcpyAsync(pr->d_layers + (ncols + c0) * 32, d_all + (size_t)q * maxn * 32, cn * 32, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
      return done(lf_fail(c, LFGPU_ERR_HIP, "ligero (sharded): leaves"));
  }
  if ((rc = lfgpu_merkle_build_tree(c, ncols, pr->d_layers, root_out))) return done(rc);
  if (verbose)
    fprintf(stderr, "lfgpu ligero column commit (sharded) rank %d/%d: rows [%zu, %zu) of %zu-byte elements: upload + RS encode + pack %.2f ms | all_to_all %.2f | leaves + all_gather + tree %.2f\n",
            rank, world, pr->row_lo, pr->row_hi, esz, tv2 - t_begin, tv3 - tv2, clock_ms() - tv3);
  return done(LFGPU_OK);
}
// The Reed-Solomon extension of rows [row_lo, row_hi) of a fresh tableau whose un-encoded image stands in d_slab: rows IDOT /
// IQUAD carry dblock values, every other row block (ligero_prover.h:175,184,203,210,237).  The dblock rows form one contiguous
// global range [idot, iquad + 1), clipped to the slab: one mixed launch where the policy has one, else group by group.
template <class L>
int extend_slab(lfgpu_ctx* c, const L& pol, const lfgpu_ligero_param& p, size_t row_lo, size_t row_hi, typename L::E* d_slab) {
  const size_t nr = row_hi - row_lo, ld = p.block_enc;
  if (nr == 0) return LFGPU_OK;
  const size_t g_lo = std::min(p.idot, p.iquad), g_hi = std::max(p.idot, p.iquad) + 1;
  if (g_hi - g_lo != 2) return lf_fail(c, LFGPU_ERR_ARG, "ligero: IDOT and IQUAD rows must be adjacent");
  const size_t lo2 = std::min(std::max(g_lo, row_lo), row_hi) - row_lo, hi2 = std::min(std::max(g_hi, row_lo), row_hi) - row_lo;
  const int rc = pol.rs_rows_mixed(c, nr, p.block, p.dblock, lo2, hi2, p.block_enc, d_slab, ld);
  if (rc != LFGPU_ERR_UNSUPPORTED) return rc;
  auto group = [&](size_t a, size_t b, size_t n) { return b > a ? pol.rs_rows(c, b - a, n, p.block_enc, d_slab + a * ld, ld) : (int)LFGPU_OK; };
  LF_TRY(group(0, lo2, p.block));
  LF_TRY(group(lo2, hi2, p.dblock));
  return group(hi2, nr, p.block);
}

// The device half of a commit: pr initialised (Slab::init, nonces drawn), H the un-encoded host image of its slab
// ([row_hi - row_lo][dblock], only the first dblock columns are ever non-trivial).  Allocates, uploads, encodes (K3/K4) and
// commits the columns (K5/K6): one GPU hashes its own columns, a sharded prover goes through the exchange above.  t_call:
// clock_ms() when the caller began its layout, for the LFGPU_VERBOSE phase lines.  Both column commits end with a stream
// synchronise, and so does every failure here: H is the caller's to scrub and free as soon as this returns.
template <class L>
int commit_rows(Slab<typename L::E>* pr, const L& pol, const typename L::E* H, double t_call, uint8_t root_out[32]) {
  constexpr size_t esz = sizeof(typename L::E);
  lfgpu_ctx* c = pr->c;
  const lfgpu_ligero_param& p = pr->p;
  const size_t nr = pr->row_hi - pr->row_lo, ld = p.block_enc;
  static const bool verbose = getenv("LFGPU_VERBOSE") != nullptr;
  const double tv1 = clock_ms();
  if (verbose && pr->sharded)
    fprintf(stderr, "lfgpu ligero_commit_sharded rank %d/%d: rows [%zu, %zu): layout + stream %.2f ms\n", pr->comm.rank, pr->comm.world, pr->row_lo, pr->row_hi, tv1 - t_call);
  auto run = [&]() -> int {
    LF_TRY(pr->alloc());
    if (nr) LF_HIP(c, hipMemcpy2DAsync(pr->d_T, ld * esz, H, p.dblock * esz, p.dblock * esz, nr, hipMemcpyHostToDevice, c->stream));
    LF_TRY(extend_slab(c, pol, p, pr->row_lo, pr->row_hi, pr->d_T));  // rows are independent: no collective
    if (pr->sharded) return column_commit_sharded(pr, pol, tv1, root_out);  // (it prints its own phases)
    // the nonces go up behind the encode: in front of it, the encoder's first-use table uploads of a new shape take other copy
    // paths in the runtime (4 more copy dispatches in the first Fp256Base commit of a context, profiles/ligero_commit/)
    void* d_non = nullptr;
    LF_TRY(lf_scratch3(c, p.block_ext * 32, &d_non));
    LF_HIP(c, hipMemcpyAsync(d_non, pr->nonces.data(), p.block_ext * 32, hipMemcpyHostToDevice, c->stream));
    double tv2 = 0;
    if (verbose) {
      (void)hipStreamSynchronize(c->stream);
      tv2 = clock_ms();
    }
    LF_TRY(lfgpu_column_commit(c, pol.field, p.nrow, ld, p.dblock, p.block_ext, pr->d_T, d_non, pr->d_layers, root_out));
    if (verbose)
      fprintf(stderr, "lfgpu ligero_commit: %zu rows x %zu (block %zu, dblock %zu): host layout + draws %.2f ms | upload + RS encode %.2f | column hash + tree %.2f\n",
              p.nrow, ld, p.block, p.dblock, tv1 - t_call, tv2 - tv1, clock_ms() - tv2);
    return LFGPU_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(c->stream);  // a copy out of H may still be pending
  return rc;
}

// ---- LigeroProver::prove for nb committed provers of one shape in one chain of dispatches (lfgpu_ligero_prove_batch / _open_batch
// and their 256 twins, and the ZK drivers).  P is the prover record: Slab<E> or a type derived from it.  Host vectors come and go as
// bytes (the C ABI's arrays are 8-byte aligned words, 32-byte elements want 16).
// What both calls ask of their provers whatever the width, found before anything is enqueued; the width's own demands follow
// (L::batch_ok, which also yields the policy: the 16-byte one carries the provers' field).
template <class P>
int batch_core(lfgpu_ctx* c, const char* who, P* const* pr, size_t nb) {
  if (nb == 0 || nb > LFGPU_SC_BATCH_MAX) return lf_fail(c, LFGPU_ERR_ARG, "%s: nb = %zu, a batch holds 1..%d statements", who, nb, LFGPU_SC_BATCH_MAX);
  for (size_t b = 0; b < nb; ++b) {
    if (!pr[b]) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu is NULL", who, b);
    if (pr[b]->c != c) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu belongs to another context", who, b);
    if (memcmp(&pr[b]->p, &pr[0]->p, sizeof(lfgpu_ligero_param)) != 0) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu has another lfgpu_ligero_param than prover 0", who, b);
    for (size_t a = 0; a < b; ++a)
      if (pr[a] == pr[b]) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu appears twice", who, b);
  }
  return LFGPU_OK;
}
// statements per launch chain: the chain's working set in scratch3 (`per` bytes a statement) stays below LF_CB_SCRATCH_CAP, and the
// chain within what the encoder of its A rows takes (rs_cap = L::batch_rs_cap); LFGPU_LP_CHUNK overrides (read once)
inline size_t batch_chunk(size_t nb, size_t per, size_t rs_cap) {
  static const long env = getenv("LFGPU_LP_CHUNK") ? atol(getenv("LFGPU_LP_CHUNK")) : 0;
  size_t chunk = std::min(std::min(nb, rs_cap), std::max<size_t>(1, LF_CB_SCRATCH_CAP / std::max<size_t>(per, 1)));
  if (env > 0) chunk = std::min(chunk, (size_t)env);
  return std::max<size_t>(chunk, 1);
}
// elements that hold n u64 words behind one another (the index lists and offset tables of the uploaded blocks)
template <class E>
constexpr size_t u64_elts(size_t n) {
  return (n * 8 + sizeof(E) - 1) / sizeof(E);
}

// low_degree_proof, dot_proof (A = scale * dense + the sparse terms, as dot builds it) and quadratic_proof of nb provers: per chain
// one upload, one memset, one dense and one sparse launch, the Reed-Solomon extension of the chain's A rows, the three
// combinations, one read-back.  Arguments as lfgpu_ligero_prove_batch (lfgpu.h).
template <class L, class P>
int prove_batch(lfgpu_ctx* c, const char* who, P* const* pr, size_t nb, const void* h_u_ldt, const void* const* d_dense, size_t ndense, const void* scale,
                const uint64_t* const* h_idx, const void* const* h_val, const size_t* nsparse, const void* h_u_quad, void* h_y_ldt, void* h_y_dot, void* h_y_q0,
                void* h_y_q2) {
  using E = typename L::E;
  constexpr size_t esz = sizeof(E);
  L pol{};
  LF_TRY(batch_core(c, who, pr, nb));
  LF_TRY(L::batch_ok(c, who, pr, nb, &pol));
  const lfgpu_ligero_param& p = pr[0]->p;
  const size_t nwq = p.nwqrow, nqt = p.nqtriples, lda = p.dblock, nflat = nwq * p.w, ymid = p.dblock - p.block;
  if ((nwq && !h_u_ldt) || (nqt && !h_u_quad) || ndense > nflat || (ndense && (!d_dense || !scale)))
    return lf_fail(c, LFGPU_ERR_ARG, "%s: null challenge vector / dense block, or ndense > nwqrow * w", who);
  if (nwq >> 31 || nqt >> 31 || p.w >> 32 || p.r >> 32) return lf_fail(c, LFGPU_ERR_ARG, "%s: too many rows", who);  // the kernels take them as u32
  for (size_t b = 0; b < nb; ++b) {
    if (ndense && !d_dense[b]) return lf_fail(c, LFGPU_ERR_ARG, "%s: dense block of statement %zu is NULL", who, b);
    if (nsparse[b] && (!h_idx || !h_val || !h_idx[b] || !h_val[b])) return lf_fail(c, LFGPU_ERR_ARG, "%s: sparse list of statement %zu is NULL", who, b);
    for (size_t t = 0; t < nsparse[b]; ++t) {
      if (h_idx[b][t] >= nflat) return lf_fail(c, LFGPU_ERR_ARG, "%s: sparse index out of range (statement %zu)", who, b);
      if (t && h_idx[b][t] <= h_idx[b][t - 1]) return lf_fail(c, LFGPU_ERR_ARG, "%s: sparse indices must be strictly increasing (statement %zu)", who, b);
    }
  }
  // the working set of a chain of cb statements in scratch3, in elements: Aext [cb][nwq][dblock] | y [cb][block + 2 dblock] (y_ldt | y_dot |
  // y_quad) | one uploaded block: u_ldt [cb][nwq] | u_quad [cb][nqt] | scale [cb] | val [tot] | idx [tot] (u64) | off [cb + 1] (u64).
  // The uploaded block stays in scratch3: scratch2 is the Reed-Solomon encoder's work space.
  const size_t sA = nwq * lda, sy = p.block + 2 * p.dblock;
  const size_t chunk = batch_chunk(nb, (sA + sy + nwq + nqt + 1) * esz, pol.batch_rs_cap(p));
  auto pack_elts = [&](size_t cb, size_t tot) { return cb * (nwq + nqt + 1) + tot + u64_elts<E>(tot) + u64_elts<E>(cb + 1); };
  size_t need = 0;
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t cb = std::min(chunk, nb - b0);
    size_t tot = 0;
    for (size_t b = b0; b < b0 + cb; ++b) tot += nsparse[b];
    need = std::max(need, (cb * (sA + sy) + pack_elts(cb, tot)) * esz + 64);
  }
  LF_HIP(c, hipSetDevice(c->device));
  // A dense block must not live in the scratch this call is about to overwrite.  Checked twice: against the buffer as it stands
  // (growing it frees that memory, so a block inside it would dangle), and against the buffer after lf_scratch3 has grown it --
  // the second refusal comes after an allocation, but still before anything is enqueued or written.  Only scratch3 is checked:
  // the RS extension below also works through scratch and scratch2, but it runs after a_rows_dense_batch, the only reader of the
  // dense blocks, in stream order -- as in dot.
  auto aliases = [&]() {
    const uint8_t* lo = (const uint8_t*)c->scratch3;
    const size_t span = c->scratch3_bytes;
    for (size_t b = 0; b < nb && ndense && lo; ++b) {
      const uint8_t* d = (const uint8_t*)d_dense[b];
      if (d + ndense * esz > lo && d < lo + span) return true;
    }
    return false;
  };
  if (aliases()) return lf_fail(c, LFGPU_ERR_ARG, "%s: a dense block aliases the call's scratch", who);
  void* sc = nullptr;
  LF_TRY(lf_scratch3(c, need, &sc));
  if (aliases()) return lf_fail(c, LFGPU_ERR_ARG, "%s: a dense block aliases the call's scratch", who);
  std::vector<E> pack, y;
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t cb = std::min(chunk, nb - b0);
    size_t tot = 0, maxsp = 0;
    for (size_t b = b0; b < b0 + cb; ++b) {
      tot += nsparse[b];
      maxsp = std::max(maxsp, nsparse[b]);
    }
    E* const dAext = (E*)sc;
    E* const dy = dAext + cb * sA;
    E* const d_pack = dy + cb * sy;
    // the host image of the uploaded block (kept until the chain's read-back has synchronised)
    pack.assign(pack_elts(cb, tot), E{});
    const size_t o_uq = cb * nwq, o_sc = o_uq + cb * nqt, o_val = o_sc + cb, o_idx = o_val + tot, o_off = o_idx + u64_elts<E>(tot);
    if (nwq) memcpy((void*)pack.data(), (const uint8_t*)h_u_ldt + b0 * nwq * esz, cb * nwq * esz);
    if (nqt) memcpy((void*)(pack.data() + o_uq), (const uint8_t*)h_u_quad + b0 * nqt * esz, cb * nqt * esz);
    if (ndense) memcpy((void*)(pack.data() + o_sc), (const uint8_t*)scale + b0 * esz, cb * esz);
    u64* const pk_idx = (u64*)(pack.data() + o_idx);
    u64* const pk_off = (u64*)(pack.data() + o_off);
    LfBatchPtrs pt{}, pd{};
    size_t run = 0;
    for (size_t b = 0; b < cb; ++b) {
      const size_t g = b0 + b;
      pk_off[b] = run;
      if (nsparse[g]) {
        memcpy((void*)(pack.data() + o_val + run), h_val[g], nsparse[g] * esz);
        memcpy(pk_idx + run, h_idx[g], nsparse[g] * 8);
      }
      run += nsparse[g];
      pt.p[b] = pr[g]->d_T;
      pd.p[b] = ndense ? const_cast<void*>(d_dense[g]) : nullptr;
    }
    pk_off[cb] = run;
    LF_HIP(c, hipMemcpyAsync(d_pack, pack.data(), pack.size() * esz, hipMemcpyHostToDevice, c->stream));
    // inner_product_vector + layout_Aext of every statement: one memset, one dense and one sparse launch
    if (cb * sA) LF_HIP(c, hipMemsetAsync(dAext, 0, cb * sA * esz, c->stream));
    if (ndense) LF_TRY(pol.a_rows_dense_batch(c, cb, p.r, p.w, lda, d_pack + o_sc, pd, ndense, dAext, sA));
    if (maxsp) LF_TRY(pol.a_rows_sparse_batch(c, cb, p.r, p.w, lda, (const u64*)(d_pack + o_idx), d_pack + o_val, (const u64*)(d_pack + o_off), maxsp, nflat, dAext, sA));
    // the A rows from block to dblock values, in place (ld = dblock)
    if (nwq) LF_TRY(pol.rs_rows_batch(c, cb, dAext, sA, nwq, p.block, p.dblock, lda));
    // dot proof and low-degree proof (y_ldt | y_dot of a statement), quadratic proof
    LF_TRY(pol.rows_combo_batch(c, cb, p, pt, dAext, sA, d_pack, dy, sy));
    LF_TRY(pol.quad_combo_batch(c, cb, p, pt, d_pack + o_uq, dy + p.block + p.dblock, sy));
    y.resize(cb * sy);
    LF_TRY(lfgpu_memcpy_d2h(c, y.data(), dy, cb * sy * esz));  // all three y vectors of all statements of the chain
    for (size_t b = 0; b < cb; ++b) {  // the reference's sanity check (:335-337), as quadratic makes it
      const E* yq = y.data() + b * sy + p.block + p.dblock;
      for (size_t j = 0; j < p.w; ++j)
        if (!pol.is_zero(yq[p.r + j])) return lf_fail(c, LFGPU_ERR_ASSERT, "quadratic_proof: W part is nonzero (statement %zu)", b0 + b);
    }
    for (size_t b = 0; b < cb; ++b) {
      const E* yb = y.data() + b * sy;
      const size_t g = b0 + b;
      memcpy((uint8_t*)h_y_ldt + g * p.block * esz, yb, p.block * esz);
      memcpy((uint8_t*)h_y_dot + g * p.dblock * esz, yb + p.block, p.dblock * esz);
      const E* yq = yb + p.block + p.dblock;
      memcpy((uint8_t*)h_y_q0 + g * p.r * esz, yq, p.r * esz);
      memcpy((uint8_t*)h_y_q2 + g * ymid * esz, yq + p.block, ymid * esz);
    }
  }
  return LFGPU_OK;
}

// compute_req + MerkleCommitment::open for nb provers: per chain the index lists of all statements in one upload, one column
// gather, one digest gather (merkle.hip's: digests do not know the field) and one read-back of the columns and the digests, which
// stand behind one another.  idx [nb][nreq]; h_req [nb][nrow][nreq]; statement b's path at h_path + b * path_cap * 32.
template <class L, class P>
int open_batch(lfgpu_ctx* c, const char* who, P* const* pr, size_t nb, const size_t* idx, void* h_req, uint8_t* h_nonces, uint8_t* h_path, size_t path_cap,
               size_t* npath) {
  using E = typename L::E;
  constexpr size_t esz = sizeof(E), dig = 32 / esz;  // elements per digest
  L pol{};
  LF_TRY(batch_core(c, who, pr, nb));
  LF_TRY(L::batch_ok(c, who, pr, nb, &pol));
  const lfgpu_ligero_param& p = pr[0]->p;
  const size_t nreq = p.nreq, nrow = p.nrow, ncols = p.block_ext;
  if (nreq == 0) return lf_fail(c, LFGPU_ERR_ARG, "%s: nreq = 0 (a proof with 0 leaves is not defined)", who);
  if ((nrow * nreq) >> 32) return lf_fail(c, LFGPU_ERR_ARG, "%s: nrow * nreq does not fit 32 bits", who);
  for (size_t b = 0; b < nb; ++b)
    if (pr[b]->nonces.size() != 32 * ncols || !pr[b]->d_layers) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu holds no commitment", who, b);
  // MerkleTree::generate_compressed_proof's walk per statement (it also rejects an index out of range or given twice)
  std::vector<u64> nodes;
  std::vector<size_t> off(nb + 1, 0);
  for (size_t b = 0; b < nb; ++b) {
    LF_TRY(lf_merkle_path_nodes(c, ncols, idx + b * nreq, nreq, nodes));
    off[b + 1] = nodes.size();
    if (off[b + 1] - off[b] > path_cap || (off[b + 1] > off[b] && !h_path)) return lf_fail(c, LFGPU_ERR_ARG, "%s: path buffer too small (statement %zu)", who, b);
  }
  LF_HIP(c, hipSetDevice(c->device));
  // a chain of cb statements in scratch3: req [cb][nrow][nreq] | digests [32 bytes per node] | idx [cb][nreq] (u64) | nodes (u64) | off [cb + 1] (u64)
  const size_t chunk = batch_chunk(nb, nrow * nreq * esz + nreq * (p.mc_pathlen + 1) * 32, pol.batch_rs_cap(p));
  auto words = [&](size_t cb, size_t tot) { return cb * nreq + tot + cb + 1; };
  size_t need = 0;
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t cb = std::min(chunk, nb - b0), tot = off[b0 + cb] - off[b0];
    need = std::max(need, (cb * nrow * nreq + dig * tot + u64_elts<E>(words(cb, tot))) * esz + 64);
  }
  void* sc = nullptr;
  LF_TRY(lf_scratch3(c, need, &sc));
  std::vector<u64> pack;
  std::vector<uint8_t> back;
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t cb = std::min(chunk, nb - b0), tot = off[b0 + cb] - off[b0];
    E* const d_req = (E*)sc;
    E* const d_dig = d_req + cb * nrow * nreq;
    u64* const d_pack = (u64*)(d_dig + dig * tot);
    pack.assign(words(cb, tot), 0);
    LfBatchPtrs pt{}, pl{};
    size_t maxcnt = 0;
    for (size_t b = 0; b < cb; ++b) {
      const size_t g = b0 + b;
      for (size_t j = 0; j < nreq; ++j) pack[b * nreq + j] = idx[g * nreq + j];
      pack[cb * nreq + tot + b] = off[g] - off[b0];
      maxcnt = std::max(maxcnt, off[g + 1] - off[g]);
      pt.p[b] = pr[g]->d_T;
      pl.p[b] = pr[g]->d_layers;
    }
    pack[cb * nreq + tot + cb] = tot;
    for (size_t t = 0; t < tot; ++t) pack[cb * nreq + t] = nodes[off[b0] + t];
    LF_HIP(c, hipMemcpyAsync(d_pack, pack.data(), pack.size() * 8, hipMemcpyHostToDevice, c->stream));
    LF_TRY(pol.gather_columns_batch(c, cb, nrow, p.block_enc, p.dblock, pt, d_pack, nreq, d_req));
    LF_TRY(lf_merkle_gather_batch(c, cb, ncols, pl, d_pack + cb * nreq, d_pack + cb * nreq + tot, maxcnt, d_dig));
    back.resize(cb * nrow * nreq * esz + tot * 32);
    LF_TRY(lfgpu_memcpy_d2h(c, back.data(), d_req, back.size()));
    memcpy((uint8_t*)h_req + b0 * nrow * nreq * esz, back.data(), cb * nrow * nreq * esz);
    const uint8_t* digests = back.data() + cb * nrow * nreq * esz;
    for (size_t b = 0; b < cb; ++b) {
      const size_t g = b0 + b, cnt = off[g + 1] - off[g];
      if (cnt) memcpy(h_path + g * path_cap * 32, digests + (off[g] - off[b0]) * 32, cnt * 32);
      npath[g] = cnt;
      for (size_t j = 0; j < nreq; ++j) memcpy(h_nonces + (g * nreq + j) * 32, &pr[g]->nonces[32 * idx[g * nreq + j]], 32);
    }
  }
  return LFGPU_OK;
}
}  // namespace
}  // namespace lig
