/* lfgpu_zk.h -- C ABI of the ZK prover host driver (the callers of the hot path).
 *
 * lfgpu.h is the kernel-level boundary; this header is one level up: the host control flow of
 *   ZkProver::commit / ZkProver::prove        lib/zk/zk_prover.h:72-149
 *   ZkCommon::verifier_constraints            lib/zk/zk_common.h:49-136,406-439
 *   LigeroProver::prove                       lib/ligero/ligero_prover.h:84-146
 *   ZkProof::write                            lib/zk/zk_proof.h:90-185
 *   CircuitRep::from_bytes (LFC1)             lib/proto/circuit.h, lib/proto/circuit_reader.h:55-233
 * written in C++ inside the library, with every data-parallel step on the device through the lfgpu.h kernels.
 * Fields: GF2_128<4> (the field of BM_ShaZK_fp2_128, lib/circuits/sha/flatsha256_circuit_test.cc:510-536; LCH14
 * Reed-Solomon) and Fp128 (field id 6; ReedSolomonFactory over FFTConvolutionFactory with the 2^32-order root, as
 * lib/zk/zk_test.cc:252-330 sets it up); other field ids in the circuit header return LFGPU_ERR_UNSUPPORTED.
 * Elements cross the ABI as the reference's in-memory Elt images (Fp128: Montgomery form) and the wire as
 * to_bytes_field images.
 *
 * The Fiat-Shamir transcript and the RandomEngine are the CALLER's: they are reached through the hooks below, so
 * an integration passes thin wrappers over proofs::Transcript / proofs::RandomEngine.  A built-in
 * transcript with the reference's exact construction (SHA-256 state + AES-256-ECB counter PRF,
 * lib/random/transcript.h:33-190) is provided for stand-alone use and for the tests.
 */
#ifndef LFGPU_ZK_H_
#define LFGPU_ZK_H_

#include "lfgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Fiat-Shamir transcript hooks (proofs::Transcript, lib/random/transcript.h:70-190) ---- */
typedef struct lfgpu_transcript_ops {
  void* user;
  /* Transcript::write(const uint8_t*, size_t): tag 0 || u64 length || bytes */
  void (*write_bytes)(void* user, const uint8_t* data, size_t n);
  /* Transcript::write(const Elt&, F): tag 1 || to_bytes_field image (elt16 = that 16-byte image) */
  void (*write_elt)(void* user, const uint8_t* elt16);
  /* Transcript::write(const Elt[], ince, n, F): tag 2 || u64 count || images */
  void (*write_elt_array)(void* user, const uint8_t* elts16, size_t n);
  /* RandomEngine::bytes: n PRF bytes */
  void (*gen_bytes)(void* user, uint8_t* out, size_t n);
  /* Transcript::clone(): a new `user` with the same state (ZkProver::prove runs the sumcheck prover on a
   * copy, zk_prover.h:117-124); release with free_clone */
  void* (*clone)(void* user);
  void (*free_clone)(void* user);
  /* the element writes for a field whose to_bytes_field image is not 16 bytes (Fp256Base, field id 1: nbytes = 32):
   * tag 1 || image[nbytes];  tag 2 || u64 count || count images.  The 16-byte fields never call them; a transcript that
   * only serves those may leave them NULL (the P-256 prover then fails with LFGPU_ERR_ARG). */
  void (*write_elt_sized)(void* user, const uint8_t* elt, size_t nbytes);
  void (*write_elt_array_sized)(void* user, const uint8_t* elts, size_t n, size_t nbytes);
} lfgpu_transcript_ops;

/* built-in transcript, byte-identical to the reference's (pinned by the ZK fixtures and FIPS-197/180-4 vectors) */
typedef struct lfgpu_transcript lfgpu_transcript;
lfgpu_transcript* lfgpu_transcript_new(const uint8_t* init, size_t n); /* Transcript(init, n) */
void lfgpu_transcript_free(lfgpu_transcript* t);
void lfgpu_transcript_get_ops(lfgpu_transcript* t, lfgpu_transcript_ops* ops);
/* direct access for tests */
void lfgpu_transcript_write_bytes(lfgpu_transcript* t, const uint8_t* data, size_t n);
void lfgpu_transcript_write_elt(lfgpu_transcript* t, const uint8_t* elt16);
void lfgpu_transcript_write_elt_array(lfgpu_transcript* t, const uint8_t* elts16, size_t n);
void lfgpu_transcript_bytes(lfgpu_transcript* t, uint8_t* out, size_t n);
/* ... for elements whose to_bytes_field image is nbytes long (Fp256Base: 32) */
void lfgpu_transcript_write_elt_sized(lfgpu_transcript* t, const uint8_t* elt, size_t nbytes);
void lfgpu_transcript_write_elt_array_sized(lfgpu_transcript* t, const uint8_t* elts, size_t n, size_t nbytes);
/* primitives the transcript is built from (known-answer tested) */
void lfgpu_sha256(const uint8_t* data, size_t n, uint8_t out[32]);
void lfgpu_aes256_ecb_block(const uint8_t key[32], const uint8_t in[16], uint8_t out[16]);
/* host-side GF(2^128) product used by the driver's bookkeeping (GF2_128::mulf, lib/gf2k/gf2_128.h:233-246):
 * PCLMULQDQ when available, portable otherwise */
void lfgpu_host_gf2128_mul(const uint64_t a[2], const uint64_t b[2], uint64_t out[2]);
/* SHA-NI / AES-NI / PCLMULQDQ dispatch: force_portable = 1 / 0 switches the portable C++ paths on / off, < 0 only queries;
 * returns 1 when the hardware paths are active. */
int lfgpu_crypto_hw(int force_portable);

/* ---- circuit (LFC1 wire format -> device-resident layers) ---- */
typedef struct lfgpu_circuit lfgpu_circuit;
typedef struct {
  int field; /* LFGPU_FIELD_* */
  size_t nv, nc, npub_in, subfield_boundary, ninputs, nl, logv, nterms;
  uint8_t id[32];
} lfgpu_circuit_info;
/* CircuitRep::from_bytes (lib/proto/circuit.h): parses the LFC1 bytes, delta-decodes every layer's corners
 * (circuit_reader.h:55-233) and uploads them with lfgpu_quad_upload.  LFGPU_ERR_ARG on malformed input.
 * The ZK entry points of this header stay at nc = 1: the reference's ZkProver requires logc = 0 (lib/zk/zk_common.h:72), so
 * a circuit with nc != 1 is LFGPU_ERR_UNSUPPORTED here.  The sumcheck over nc > 1 copies is in the kernel-level ABI
 * (lfgpu_eval_quad_copies, lfgpu_sumcheck_layer_copies in lfgpu.h). */
int lfgpu_circuit_from_lfc1(lfgpu_ctx* ctx, const uint8_t* bytes, size_t len, lfgpu_circuit** out);
/* A second handle on the same uploaded circuit for ANOTHER context of the same device (throughput mode: K host threads, each
 * with its own context -- lfgpu_own_stream -- prover and transcript, one copy of the circuit in HBM).  The device arrays are
 * reference-counted: the handles may be freed in any order.  `src` must not be in use by another thread during the call. */
int lfgpu_circuit_share(lfgpu_ctx* ctx, const lfgpu_circuit* src, lfgpu_circuit** out);
int lfgpu_circuit_get_info(const lfgpu_circuit* c, lfgpu_circuit_info* info);
int lfgpu_circuit_layer_info(const lfgpu_circuit* c, size_t layer, size_t* logw, size_t* nw, size_t* nterms);
int lfgpu_circuit_free(lfgpu_circuit* c);

/* ---- ZkProver ---- */
typedef struct lfgpu_zk_prover lfgpu_zk_prover;
/* ZkProver(c, F, rsf) + ZkProof(c, rateinv, nreq[, block_enc]) (zk_proof.h:63-76): block_enc = 0 searches. */
int lfgpu_zk_prover_new(lfgpu_ctx* ctx, const lfgpu_circuit* c, size_t rateinv, size_t nreq, size_t block_enc,
                        lfgpu_zk_prover** out);
int lfgpu_zk_prover_param(const lfgpu_zk_prover* zk, lfgpu_ligero_param* p);
/* More than one GPU behind the same prover (BASELINE config 5 names it).  Every rank constructs the prover on its
 * own device and calls commit / prove / proof_write with the same arguments and its own copy of the transcript (SPMD); `rng`
 * is only drawn from on rank 0 (its stream is broadcast).  A Ligero tableau of at least min_tableau_bytes is committed with
 * its rows sharded over the communicator's GPUs (lfgpu_ligero_commit_sharded in lfgpu.h: one all_to_all + one all_gather per
 * commit, field-sum folds of the y vectors in prove); below the threshold the proof runs replicated, which is what the
 * real mdoc / flatsha256 circuits want (their tableaux are 2.5 - 20 MB: a second GPU only adds latency -- use independent
 * proofs per GPU instead, lfgpu_own_stream / bench.py zk_throughput).  The sumcheck always runs replicated.  Every rank ends
 * with the same proof bytes as a one-GPU prover fed the same RandomEngine.  comm = NULL: back to one GPU.  All three
 * fields (the mdoc signature circuit over Fp256Base has a 2.5 MB tableau: leave it replicated). */
int lfgpu_zk_prover_set_comm(lfgpu_zk_prover* zk, const lfgpu_comm_ops* comm, size_t min_tableau_bytes);
/* ZkProver::commit (zk_prover.h:72-96): fill_pad from `rng`, Ligero-commit witness||pad, root -> transcript.
 * h_W: ninputs host elements (public inputs first). */
int lfgpu_zk_commit(lfgpu_zk_prover* zk, const void* h_W, lfgpu_rng_fn rng, void* rng_user,
                    const lfgpu_transcript_ops* ts, uint8_t root_out[32]);
/* ZkProver::prove (zk_prover.h:98-149): *ok = 0 when the witness does not satisfy the circuit (the reference
 * returns false); otherwise the proof is held by the prover object. */
int lfgpu_zk_prove(lfgpu_zk_prover* zk, const void* h_W, const lfgpu_transcript_ops* ts, int* ok);
/* ZkProof::write (zk_proof.h:90-185): the wire bytes of commitment || sumcheck proof || Ligero proof.
 * Call with buf = NULL to get the size. */
int lfgpu_zk_proof_write(const lfgpu_zk_prover* zk, uint8_t* buf, size_t cap, size_t* nbytes);
/* host milliseconds spent in the last commit / prove, split by phase:
 * [0] commit total, [1] prove total, [2] eval_circuit, [3] sumcheck, [4] constraints, [5] ligero prove */
int lfgpu_zk_timings(const lfgpu_zk_prover* zk, double ms[6]);
/* Lifetimes: a prover may be FREED after its circuit (the scrub of its device buffers goes by the byte sizes recorded when they
 * were allocated, not by the circuit handle), but not USED after it: commit, prove and proof_write read the circuit.  The
 * context must outlive both. */
int lfgpu_zk_prover_free(lfgpu_zk_prover* zk);

/* ---- ZkProver::prove for a batch of committed provers ----
 * nb provers of ONE context and ONE circuit, each committed by lfgpu_zk_commit with its own witness, RandomEngine and
 * transcript, go through ONE chain of dispatches: eval_circuit is one launch per layer for all statements
 * (lfgpu_eval_quad_batch) and the padded sumcheck one lfgpu_sumcheck_layer_batch call per layer.  Then, for the statements
 * with a good witness: the constraints per statement on the host, ONE launch for the EQ tables of their input constraints, ONE
 * lfgpu_ligero_prove_batch and ONE lfgpu_ligero_open_batch (lfgpu.h) -- three synchronising read-backs per chunk of
 * statements (lfgpu.h: LFGPU_LP_CHUNK), normally one chunk.
 * LFGPU_LIGERO_PROVE_BATCH=0 (read once per process; the A/B switch, the same bytes) runs constraints, Ligero prove and
 * opening per statement, one after the other, with the code of lfgpu_zk_prove; so does a batch whose good statements do not all
 * hold the same lfgpu_ligero_param -- provers of one circuit made with different rate, nreq or block_enc: a valid batch, the
 * sumcheck does not depend on them, but their tableaux differ in shape.  Statement b's proof is
 * byte-identical to what lfgpu_zk_prove(zk[b], h_W[b], ts[b]) produces and ts[b] is left in the same state; afterwards every
 * prover holds its own proof (lfgpu_zk_proof_write, lfgpu_zk_timings as before).  ok[b] = 0 when witness b does not satisfy the
 * circuit: that prover holds no proof, the others are unaffected.
 * lfgpu_zk_timings after a batch: [2] eval_circuit and [3] sumcheck are the BATCH's phase times and [1] the whole call's, the
 * same values for every member; so are [4] constraints and [5] Ligero prove on the batched path (the batch's phase times: the
 * statements' device work is one chain); with LFGPU_LIGERO_PROVE_BATCH=0, or in a batch of mixed Ligero parameters, those two
 * stay the statement's own.  [0] is its commit's.
 * An error code from the call (not ok[b] = 0, which is a result) leaves the batch without a usable outcome: on the batched path
 * an error in the tail -- for example LFGPU_ERR_ASSERT for one statement's y_quad -- leaves EVERY statement without a proof and
 * with ok[b] = 0, where the per-statement loop has already completed the statements in front of the failing one.
 * The batch object owns the device memory the lock-step needs nb_max times (the layers' inputs, the outputs, their pinned
 * read-back, the EQ tables over the inputs), allocated once in lfgpu_zk_batch_new.  lfgpu_zk_prove_batch frees no device
 * memory; what it may allocate is the context's pooled scratch, which grows on the first call at a shape and is kept.  The
 * slabs that hold functions of the witnesses are scrubbed when the batch is freed (the EQ tables depend on challenges only).
 * The batch may be freed before or after the provers, and like a prover after the circuit (but not used after it); the
 * context must outlive it.  The same holds for lfgpu_zk_batch256.
 * The library stays single-threaded per call: the host work per statement -- the Fiat-Shamir preamble (SHA-256 over nterms
 * zero bytes), the constraints, proof_write -- is serial inside one batch.  A caller that wants more throughput runs several
 * batches in several contexts (lfgpu_own_stream, lfgpu_circuit_share), as examples/zk_throughput.cc does with provers.
 * 1 <= nb <= nb_max <= LFGPU_SC_BATCH_MAX.  LFGPU_ERR_ARG: a NULL argument, nb out of range, a prover of another context or
 * circuit, one that has not committed, the same prover twice.  LFGPU_ERR_UNSUPPORTED: an Fp256Base circuit (at _new: those
 * take lfgpu_zk_batch256_new / lfgpu_zk_prove_batch256 below), a prover with a communicator set.  LFGPU_ERR_NOMEM from _new when
 * the slabs do not fit. */
typedef struct lfgpu_zk_batch lfgpu_zk_batch;
int lfgpu_zk_batch_new(lfgpu_ctx* ctx, const lfgpu_circuit* c, size_t nb_max, lfgpu_zk_batch** out);
int lfgpu_zk_prove_batch(lfgpu_zk_batch* batch, lfgpu_zk_prover* const* zk, size_t nb, const void* const* h_W,
                         const lfgpu_transcript_ops* const* ts, int* ok /*[nb]*/);
int lfgpu_zk_batch_free(lfgpu_zk_batch* batch);
/* ---- the same over Fp256Base (circuits with field id LFGPU_FIELD_P256) ----
 * The contract of lfgpu_zk_prove_batch with 32-byte Montgomery images, under names of its own (the three calls above keep
 * refusing the field): nb provers of ONE context and ONE Fp256Base circuit, each committed by lfgpu_zk_commit, through one
 * chain -- lfgpu_eval_quad_batch256's two launches per layer, one lfgpu_sumcheck_layer_batch256 per layer, then for the
 * statements with a good witness the constraints per statement on the host, ONE launch chain for the EQ tables of their input
 * constraints (the public parts of all tables back in one copy), ONE lfgpu_ligero_prove_batch256 and ONE
 * lfgpu_ligero_open_batch256 (lfgpu.h).  Statement b's proof is byte-identical to lfgpu_zk_prove(zk[b], h_W[b], ts[b]) and
 * ts[b] is left in the same state; ok[b] = 0 for a bad witness: that prover holds no proof, the others are unaffected.
 * LFGPU_LIGERO_PROVE_BATCH256=0 (read once per process; the 16-byte fields keep LFGPU_LIGERO_PROVE_BATCH) runs constraints,
 * Ligero prove and opening per statement with the code of lfgpu_zk_prove: the same bytes; so does a batch whose good statements
 * hold different lfgpu_ligero_param.  lfgpu_zk_timings: [2] and [3] are the batch's phase times, the same values for every
 * member, [1] the whole call's; [4] and [5] the batch's on the batched tail and the statement's own otherwise.  Errors in the
 * tail, the batch object's memory (allocated once in _new, the witness-dependent slabs scrubbed on free, no hipMalloc / hipFree
 * in the prove call beyond the context's pooled scratch) and the threading model: as above.
 * The commit of the batch's provers in one chain is lfgpu_zk_commit_batch256 below.  Not batched for this field: the verifier,
 * and there is no resident grid for the batch's sumcheck.
 * 1 <= nb <= nb_max <= LFGPU_SC_BATCH_MAX.  LFGPU_ERR_ARG, found before anything is enqueued or any transcript is touched: a
 * NULL argument, nb out of range, a prover of another context or circuit, one that has not committed, the same prover twice, a
 * transcript without write_elt_sized / write_elt_array_sized, at _new a circuit over a 16-byte field (lfgpu_zk_batch_new serves
 * those).  LFGPU_ERR_UNSUPPORTED: a prover with a communicator set.  LFGPU_ERR_NOMEM from _new when the slabs do not fit. */
typedef struct lfgpu_zk_batch256 lfgpu_zk_batch256;
int lfgpu_zk_batch256_new(lfgpu_ctx* ctx, const lfgpu_circuit* c, size_t nb_max, lfgpu_zk_batch256** out);
int lfgpu_zk_prove_batch256(lfgpu_zk_batch256* batch, lfgpu_zk_prover* const* zk, size_t nb, const void* const* h_W,
                            const lfgpu_transcript_ops* const* ts, int* ok /*[nb]*/);
int lfgpu_zk_batch256_free(lfgpu_zk_batch256* batch);
/* ---- ZkProver::commit for a batch of provers ----
 * lfgpu_zk_commit (its one-GPU branch) for nb provers of the batch's context and circuit in one chain of dispatches: per
 * statement, in index order, fill_pad from rng[b] (its draws come before its Ligero draws, as in lfgpu_zk_commit); then ONE
 * lfgpu_ligero_commit_batch (lfgpu.h) for all statements; then, once every root is back, ts[b]->write_bytes(root b) per
 * statement.  Afterwards prover b is in exactly the state lfgpu_zk_commit leaves it in (an earlier commitment and proof are
 * dropped), so lfgpu_zk_prove or lfgpu_zk_prove_batch may follow; roots and proofs are byte-identical to the single path's.
 * lfgpu_zk_timings()[0] is the whole call's time, the same value for every member.  rng_user = NULL: every user is NULL.
 * Every statement needs a RandomEngine of its own: the pads of ALL statements are drawn before the first Ligero layout, so an
 * engine shared between statements would not see the draw order of sequential lfgpu_zk_commit calls.
 * roots_out: [nb][32] or NULL.  LFGPU_COMMIT_BATCH=0 (read once per process) runs the single-statement device path per
 * statement instead: the same bytes (the A/B switch).
 * LFGPU_ERR_ARG (found before the first draw, nothing touched): a NULL entry, nb out of 1 .. nb_max, a prover of another
 * context or circuit, the same prover twice, provers whose lfgpu_ligero_param differ (another rate, nreq or block_enc).
 * LFGPU_ERR_UNSUPPORTED: a prover with a communicator set.  On an error after the draws began no transcript has been written
 * to and every prover of the call holds no commitment. */
int lfgpu_zk_commit_batch(lfgpu_zk_batch* batch, lfgpu_zk_prover* const* zk, size_t nb, const void* const* h_W,
                          const lfgpu_rng_fn* rng, void* const* rng_user,
                          const lfgpu_transcript_ops* const* ts, uint8_t* roots_out /*[nb][32], may be NULL*/);
/* ... over Fp256Base: lfgpu_zk_commit's one-GPU branch for nb provers of the batch's context and (Fp256Base) circuit.  The same
 * contract with 32-byte Montgomery images: per statement, in index order, the pads from rng[b] (in bulk, or one call per draw
 * under lfgpu_set_rng_exact_calls) and the witness layout; then ONE lfgpu_ligero_commit_batch256 (lfgpu.h); then, once every
 * root is back, ts[b]->write_bytes(root b).  Prover b is then in exactly the state lfgpu_zk_commit leaves it in (an earlier
 * commitment and proof are dropped): lfgpu_zk_prove or lfgpu_zk_prove_batch256 may follow, and roots and proofs are
 * byte-identical to the single path's.  lfgpu_zk_timings()[0] is the whole call's time, the same value for every member.
 * Every statement needs a RandomEngine of its own, as above.  roots_out: [nb][32] or NULL.  LFGPU_COMMIT_BATCH256=0 (read once
 * per process) runs the single-statement device path per statement instead: the same bytes.
 * LFGPU_ERR_ARG (found before the first draw, nothing touched): a NULL entry, nb out of 1 .. nb_max, a prover of another
 * context or circuit or of a 16-byte field, the same prover twice, provers whose lfgpu_ligero_param differ, a transcript
 * without write_elt_sized / write_elt_array_sized (lfgpu_zk_commit refuses that too).  LFGPU_ERR_UNSUPPORTED: a prover with a
 * communicator set.  On an error after the draws began no transcript has been written to and every prover of the call holds no
 * commitment. */
int lfgpu_zk_commit_batch256(lfgpu_zk_batch256* batch, lfgpu_zk_prover* const* zk, size_t nb, const void* const* h_W,
                             const lfgpu_rng_fn* rng, void* const* rng_user,
                             const lfgpu_transcript_ops* const* ts, uint8_t* roots_out /*[nb][32], may be NULL*/);

/* ---- ZkVerifier ----
 * ZkVerifier::recv_commitment + verify (lib/zk/zk_verifier.h:68-94) on the wire bytes of ZkProof::write
 * (parsed as ZkProof::read does, lib/zk/zk_proof.h:107-112,218-345).  h_pub: the npub_in public inputs.
 * *ok = 1 iff the proof is accepted; *why (optional) names the failing check with the reference's strings
 * (lib/ligero/ligero_verifier.h:90-130) or "proof does not parse".  The transcript must be in the same
 * state the prover's was before its commit (e.g. a fresh Transcript over the same seed). */
int lfgpu_zk_verify(lfgpu_ctx* ctx, const lfgpu_circuit* c, size_t rateinv, size_t nreq, size_t block_enc,
                    const uint8_t* proof, size_t proof_len, const void* h_pub, const lfgpu_transcript_ops* ts, int* ok,
                    const char** why);

/* The same with ZkVerifier::recv_commitment already done by the caller (the commitment root -- the first 32 proof bytes --
 * written to the transcript with write_bytes): the reference keeps the two calls apart, and run_mdoc_verifier receives both
 * commitments and draws its MAC key before it verifies either proof (lib/circuits/mdoc/mdoc_zk.cc:676-681,704-705). */
int lfgpu_zk_verify_committed(lfgpu_ctx* ctx, const lfgpu_circuit* c, size_t rateinv, size_t nreq, size_t block_enc,
                              const uint8_t* proof, size_t proof_len, const void* h_pub, const lfgpu_transcript_ops* ts,
                              int* ok, const char** why);

/* ---- LigeroProver::prove / LigeroVerifier::verify on a caller's own statement ----
 * The Ligero seam without a circuit: the caller brings the linear constraints A w = b as a list of terms and the quadratic
 * constraints W[z] = W[x] W[y] as lqc, exactly what the reference's classes take.  Fields: GF2_128 (subfield_log_bits 4 or 5)
 * and Fp128.  Transcript order, as the reference's (lib/ligero/ligero_prover.h:84-146, ligero_verifier.h:42-123):
 * write hash_of_llterm; draw u_ldt[nwqrow], alphal[nl], alphaq[nq][3], u_quad[nqtriples]; write y_ldt, y_dot, y_quad_0,
 * y_quad_2; choose(block_ext, nreq).
 * The matrix of the dot proof is accumulated on the device from the term list AS GIVEN: any order, duplicates allowed
 * (inner_product_vector, ligero_param.h:382-421); the result does not depend on the order of the terms.
 * LFGPU_ERR_ARG, found on the host before the first transcript call or launch: a NULL argument (llterm may be NULL when
 * nllterm = 0, h_lqc when nq = 0, h_b when nl = 0), a term with c >= nl or w >= nw, an lqc index >= nw,
 * nllterm + 6 nq >= 2^32 (the Fp128 accumulators are 64-bit sums of 32-bit limbs), field P256 or a P-256 prover (those take
 * lfgpu_ligero_prove256 / lfgpu_ligero_verify256 below).
 * LFGPU_ERR_UNSUPPORTED: a sharded prover, or one from lfgpu_ligero_prover_from_slab. */
typedef struct { size_t c, w; uint64_t k[2]; } lfgpu_ligero_llterm;   /* LigeroLinearConstraint: A[c][w] += k */

/* LigeroProver::prove on a prover from lfgpu_ligero_commit, whose root the caller has written to ts
 * (LigeroTranscript::write_commitment).  proof: the write_com_proof bytes (lib/zk/zk_proof.h:137-185); buf = NULL asks for the
 * size.  The size depends on the proof (subfield runs, Merkle path), so the size query RUNS the proof -- ts advances -- and the
 * prover keeps the serialised bytes; the next call with a buffer copies those bytes and leaves ts alone (one proof, one
 * serialisation, as lfgpu_zk_proof_write).  A call with a buffer and no size query in front of it proves and copies in one go.
 * cap too small: LFGPU_ERR_ARG with *nbytes set, the bytes stay held for the next call with a buffer. */
int lfgpu_ligero_prove(lfgpu_ligero_prover* pr, const lfgpu_transcript_ops* ts, size_t nl, size_t nllterm,
                       const lfgpu_ligero_llterm* llterm, const uint8_t hash_of_llterm[32], const size_t* h_lqc,
                       uint8_t* buf, size_t cap, size_t* nbytes);
/* LigeroVerifier::verify after receive_commitment (root already in ts).  *ok, *why as lfgpu_zk_verify. */
int lfgpu_ligero_verify(lfgpu_ctx* ctx, int field, int subfield_log_bits, const lfgpu_ligero_param* p,
                        const uint8_t root[32], const uint8_t* proof, size_t proof_len, const lfgpu_transcript_ops* ts,
                        size_t nl, size_t nllterm, const lfgpu_ligero_llterm* llterm, const uint8_t hash_of_llterm[32],
                        const void* h_b, const size_t* h_lqc, int* ok, const char** why);


/* ---- the same two over Fp256Base (LFGPU_FIELD_P256) ----
 * A P-256 coefficient does not fit the 16-byte term record, so the field has names of its own; everything else is as above:
 * the transcript order, the size-query protocol (a size query RUNS the proof, ts advances, the bytes are held for the copy),
 * the reference's *why strings and "proof does not parse".  pr comes from lfgpu_ligero_commit(field = LFGPU_FIELD_P256); k, h_b
 * and every element on the wire are 32-byte Montgomery images; the elements go to the transcript through write_elt_array_sized
 * with nbytes = 32.  The matrix of the dot proof is accumulated on the device from the 48-byte records AS GIVEN (one upload),
 * exact and independent of their order: every product k * alphal[c] is added as eight 32-bit limbs into 64-bit integer
 * accumulators of its entry A[w] and reduced once.  SUMMAND BOUND: an entry may take every term and both copy terms of every
 * quadratic triple; the reduction (fp256_reduce_limbs) needs each 64-bit limb sum to hold (N <= 2^32 summands) and the part of
 * the sum above 2^256 to stay below 2^40 (N <= 2^40), so a statement with nllterm + 6 nq >= 2^32 is refused.
 * LFGPU_ERR_ARG, found on the host before the first transcript call or launch: a NULL argument (llterm may be NULL when
 * nllterm = 0, h_lqc when nq = 0, h_b when nl = 0), a term with c >= nl or w >= nw, an lqc index >= nw, the summand bound, a
 * transcript without write_elt_sized / write_elt_array_sized, lfgpu_ligero_prove256 on a prover of a 16-byte field (and
 * lfgpu_ligero_prove on a P-256 prover). */
typedef struct { size_t c, w; uint64_t k[4]; } lfgpu_ligero_llterm256; /* A[c][w] += k, k a 32-byte Montgomery image */
int lfgpu_ligero_prove256(lfgpu_ligero_prover* pr, const lfgpu_transcript_ops* ts, size_t nl, size_t nllterm,
                          const lfgpu_ligero_llterm256* llterm, const uint8_t hash_of_llterm[32], const size_t* h_lqc,
                          uint8_t* buf, size_t cap, size_t* nbytes);
int lfgpu_ligero_verify256(lfgpu_ctx* ctx, const lfgpu_ligero_param* p, const uint8_t root[32], const uint8_t* proof,
                           size_t proof_len, const lfgpu_transcript_ops* ts, size_t nl, size_t nllterm,
                           const lfgpu_ligero_llterm256* llterm, const uint8_t hash_of_llterm[32], const void* h_b,
                           const size_t* h_lqc, int* ok, const char** why);

#ifdef __cplusplus
}
#endif
#endif /* LFGPU_ZK_H_ */
