// zkint.h -- what zk.hip (the 16-byte fields) and zk256.hip (Fp256Base, 32-byte elements) share below the C ABI.
#pragma once
#include <memory>
#include <vector>

#include "../../include/lfgpu_zk.h"
#include "ctx.h"
#include "quad.h"

struct lfgpu_circuit {
  lfgpu_ctx* c = nullptr;
  lfgpu_circuit_info info{};
  struct Layer {
    size_t logw, nw, nterms;
    lfgpu_quad* q;
  };
  std::vector<Layer> layers;
  // nterms zero bytes: what initialize_sumcheck_fiat_shamir hashes per proof (zk_common.h:177-179); shared by the handles of lfgpu_circuit_share
  std::shared_ptr<const std::vector<uint8_t>> zeros;
  ~lfgpu_circuit() {
    for (auto& l : layers)
      if (l.q) lfgpu_quad_free(l.q);
  }
};

// ---- zk256.hip: ZkProver<Fp256Base, .> (BASELINE config 5, the mdoc signature circuit).  The policy P32, the Ligero policy L32
// and the kernels never leave that file, so these functions are where the driver layer of zk_driver.h is instantiated for them:
// Zk256 is zkp::Prover<P32>, Zk256Batch is zkp::Batch<P32>, each function one call of the generic one.  The entry points of
// zk.hip dispatch here on the circuit's field id, after their NULL checks and, for a batch, zkp::check_batch_call.
struct Zk256;
struct Zk256Batch;
int zk256_new(lfgpu_ctx* c, const lfgpu_circuit* C, size_t rateinv, size_t nreq, size_t block_enc, Zk256** out);
int zk256_param(const Zk256* z, lfgpu_ligero_param* p);
// draws_only: every RandomEngine draw of the commit and nothing else (rank 0 of a communicator, lfgpu_zk_commit)
int zk256_commit(Zk256* z, const void* h_W, lfgpu_rng_fn rng, void* rng_user, const lfgpu_transcript_ops* ts, uint8_t root_out[32], bool draws_only = false);
int zk256_prove(Zk256* z, const void* h_W, const lfgpu_transcript_ops* ts, int* ok);
int zk256_proof_write(const Zk256* z, uint8_t* buf, size_t cap, size_t* nbytes);
int zk256_timings(const Zk256* z, double ms[6]);
void zk256_free(Zk256* z);
void zk256_set_comm(Zk256* z, const lfgpu_comm_ops* comm, size_t min_tableau_bytes);  // comm == nullptr: one GPU
const lfgpu_comm_ops* zk256_comm(const Zk256* z);                                      // nullptr: none set
int zk256_batch_new(lfgpu_ctx* c, const lfgpu_circuit* C, size_t nb_max, Zk256Batch** out);
int zk256_prove_batch(Zk256Batch* bt, Zk256* const* z, size_t nb, const void* const* h_W, const lfgpu_transcript_ops* const* ts, int* ok);
int zk256_commit_batch(Zk256Batch* bt, Zk256* const* z, size_t nb, const void* const* h_W, const lfgpu_rng_fn* rng, void* const* rng_user,
                       const lfgpu_transcript_ops* const* ts, uint8_t* roots_out);
void zk256_batch_free(Zk256Batch* bt);
int zk256_verify(lfgpu_ctx* c, const lfgpu_circuit* C, size_t rateinv, size_t nreq, size_t block_enc, const uint8_t* proof, size_t proof_len, const void* h_pub,
                 const lfgpu_transcript_ops* ts, bool committed, int* ok, const char** why);
// MerkleTreeVerifier::verify_compressed_proof (lib/merkle/merkle_tree.h:160-209), host (zk.hip)
bool lf_merkle_verify(size_t n, const uint8_t root[32], const uint8_t* path, size_t npath, const uint8_t* leaves, const size_t* pos, size_t np);
// ---- ligero.hip: what lfgpu_ligero_prove / lfgpu_ligero_verify (zk.hip) need below the C ABI.
// inner_product_vector's inputs (lib/ligero/ligero_param.h:382-421), all on the host and already validated: term[t].c < nl,
// term[t].w < nw, lqc[.] < nw, nterm + 6 nq < 2^32.  The term list may come in any order and hold duplicates.
struct LfLigeroTerms {
  const lfgpu_ligero_llterm* term;
  size_t nterm;
  const elt_t* alphal;  // [nl]
  size_t nl;
  const size_t* lqc;    // [nq][3]
  const elt_t* alphaq;  // [nq][3]
};
// rows[i][r + j] += A[i * w + j] for the nwqrow rows [0^r | A_i] at stride ld of parameter set p (the dense part, if any, is there)
int lf_ligero_a_rows_terms(lfgpu_ctx* c, int field, const lfgpu_ligero_param* p, size_t ld, const LfLigeroTerms* t, void* d_rows);
// dot_proof with A = inner_product_vector(terms), on a prover that holds the whole tableau
int lf_ligero_dot_terms(lfgpu_ligero_prover* pr, const LfLigeroTerms* t, void* h_y);
// ---- zk256.hip: the Ligero prover over Fp256Base behind the kernel-level ABI.  lfgpu_ligero_prover (ligero.hip) carries one of
// these for field P256 and forwards its entry points here; the record itself (lig::Slab over 32-byte elements) and its policy
// never leave zk256.hip, so the handle is opaque.  Arguments are already checked for NULL; all host vectors are 32-byte
// Montgomery elements.
struct Lig256;
int lf_lig256_commit(lfgpu_ctx* c, const lfgpu_ligero_param* p, const void* h_W, const size_t* h_lqc, lfgpu_rng_fn rng, void* user, uint8_t root[32],
                     Lig256** out);
// nb commits of one shape in one chain of dispatches (lfgpu_ligero_commit_batch256): out[b] = statement b's record, or every
// entry NULL on an error
int lf_lig256_commit_batch(lfgpu_ctx* c, const lfgpu_ligero_param* p, size_t nb, const void* const* h_W, const size_t* h_lqc, const lfgpu_rng_fn* rng,
                           void* const* rng_user, uint8_t* roots, Lig256** out);
void lf_lig256_free(Lig256* L);
void* lf_lig256_tableau(Lig256* L);
int lf_lig256_low_degree(Lig256* L, const void* h_u, void* h_y);
int lf_lig256_dot_dense(Lig256* L, const void* h_A, void* h_y);  // A: nwqrow x w
int lf_lig256_quadratic(Lig256* L, const void* h_u, void* h_y0, void* h_y2);
int lf_lig256_open(Lig256* L, const size_t* idx, void* h_req, uint8_t* h_nonces, uint8_t* h_path, size_t path_cap, size_t* npath);
// the A step of the dot proof alone (tools/bench_ligero_a_step256.hip): rows[i][r + j] += A[i * w + j] at stride ld, with A
// accumulated on the device from a validated term list (L32::a_rows_terms), or scattered from a host-folded list of strictly
// increasing flat indices (lig::a_rows, the route of the ZK paths)
int lf_lig256_a_rows_terms(lfgpu_ctx* c, const lfgpu_ligero_param* p, size_t ld, const lfgpu_ligero_llterm256* term, size_t nterm, const void* h_alphal, size_t nl,
                           const size_t* h_lqc, const void* h_alphaq, void* d_rows);
int lf_lig256_a_rows_sparse(lfgpu_ctx* c, const lfgpu_ligero_param* p, size_t ld, const uint64_t* h_idx, const void* h_val, size_t n, void* d_rows);
struct LfLigeroView {
  lfgpu_ctx* c;
  int field, k;
  lfgpu_ligero_param p;
  bool whole;                  // one GPU, all rows: not sharded, not from a slab
  std::vector<uint8_t>* wire;  // the write_com_proof bytes a size query of lfgpu_ligero_prove / lfgpu_ligero_prove256 left behind
  bool* wire_held;
  Lig256* lig256;              // field P256: the prover's 32-byte slab; null for the 16-byte fields
};
void lf_ligero_prover_view(lfgpu_ligero_prover* pr, LfLigeroView* v);
// K11 over 32-byte elements (quad.hip forwards field 1 here)
int lf256_eval_quad_async(lfgpu_quad* q, const void* d_W, void* d_V, int* d_fail);
// ... for nb statements in two launches (the asynchronous twin of lfgpu_eval_quad_batch256): statement b's wires at d_W + b * ldw,
// its outputs at d_V + b * ldv (32-byte elements), its assert-zero failures ORed into d_fail[b]; arguments already checked
int lf256_eval_quad_batch_async(lfgpu_quad* q, size_t nb, const void* d_W, size_t ldw, void* d_V, size_t ldv, int* d_fail);
