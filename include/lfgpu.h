/*
 * lfgpu.h -- C ABI of the MI355X (gfx950) prover hot path for longfellow-zk.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Every entry point names the reference interface it replaces
 * (paths relative to the reference checkout, /root/reference in the build
 * container).  Header-only C++ adapters that present the reference's template
 * seams (ReedSolomonFactory, MerkleCommitment, ProverLayers round body) on top
 * of this ABI are in include/lfgpu_adapters.h; INTEGRATION.md shows the binding a
 * reference maintainer would add.
 *
 * Conventions
 *  - All functions return LFGPU_OK (0) or an error code; nothing aborts
 *    (the reference's check() -> abort(), lib/util/panic.h:27-37, becomes a
 *    status).  lfgpu_last_error() returns a message for the last failure.
 *  - Field elements are the reference's in-memory Elt images, 16 bytes:
 *      field 4 (GF2_128): 2 x u64 LE, polynomial basis (lib/gf2k/gf2_128.h:64-89)
 *      field 6 (Fp128)  : 2 x u64 LE, Montgomery form R = 2^128 (lib/algebra/fp_generic.h:66-78)
 *    field 1 (P256, Fp256Base) elements are 32 bytes: 4 x u64 LE, Montgomery form R = 2^256.
 *    so adapters can pass &tableau_[0] straight through.
 *  - Pointers named d_* are DEVICE pointers (HIP); h_* are host pointers.
 *    The *_host variants stage through device memory owned by the context.
 *  - Work is enqueued on the context's stream; functions that return data to
 *    host memory synchronise that stream before returning.
 *  - ld / strides are in ELEMENTS (16 bytes), not bytes.
 */
#ifndef LFGPU_H_
#define LFGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFGPU_OK 0
#define LFGPU_ERR_ARG 1         /* bad argument (null, size, alignment) */
#define LFGPU_ERR_HIP 2         /* HIP runtime error */
#define LFGPU_ERR_UNSUPPORTED 3 /* valid request outside what this build covers */
#define LFGPU_ERR_NOMEM 4
#define LFGPU_ERR_ASSERT 5      /* a reference check() would have failed (e.g. assert-zero term) */
#define LFGPU_ERR_BUSY 6        /* the device could not place a resident kernel's workgroups together (another tenant holds
                                   CUs); the prover-level entry points handle it themselves by falling back to per-launch
                                   kernels -- only a direct caller of the resident-kernel internals can see it */

#define LFGPU_FIELD_GF2_128 4 /* FieldID, lib/proto/circuit_io.h:24-36 */
#define LFGPU_FIELD_FP128 6
#define LFGPU_FIELD_P256 1 /* Fp256Base, the P-256 base field: 32-byte elements (lib/algebra/fp_p256.h); accepted by
                              lfgpu_fp256_rs_encode_rows[_host], lfgpu_column_commit[_host] / lfgpu_column_leaves,
                              lfgpu_field_binop, lfgpu_quad_upload (kvec: 32-byte elements), the Ligero prover of one GPU
                              (lfgpu_ligero_layout_rows, _commit, _low_degree_proof, _dot_proof, _quadratic_proof, _open,
                              _tableau, _free; lfgpu_ligero_prove256 / _verify256 in lfgpu_zk.h; subfield_log_bits and
                              subfield_boundary are ignored) and the whole prover-level ABI of lfgpu_zk.h (circuits with
                              field id 1); ld / n then count 32-byte elements, and host elements are 32-byte Montgomery
                              images.  The other Ligero entry points refuse the field, or a prover made over it, on the host
                              before any launch: commit_batch, commit_sharded, layout_rows_sharded, encode_rows,
                              prover_from_slab, dot_proof_sparse (LFGPU_ERR_ARG); inner_product_rows, prove_batch, open_batch
                              (LFGPU_ERR_UNSUPPORTED; an Fp256Base prover takes lfgpu_ligero_prove_batch256 /
                              lfgpu_ligero_open_batch256; the batched commit of the field is lfgpu_column_commit_batch256 /
                              lfgpu_ligero_commit_batch256, and lfgpu_zk_batch256_new / lfgpu_zk_commit_batch256 /
                              lfgpu_zk_prove_batch256 in lfgpu_zk.h are the batched prover of such a circuit).  The per-step
                              sumcheck entry points below (partials, scatter, binds, bind_g, sumcheck_layer) take the
                              16-byte fields only: for Fp256Base those steps run inside lfgpu_zk_prove / lfgpu_zk_verify, and
                              the whole layer has entry points of its own: lfgpu_sumcheck_layer256,
                              lfgpu_sumcheck_layer_batch256 and lfgpu_eval_quad_batch256 */

typedef struct lfgpu_ctx lfgpu_ctx;

/* ---- context ---------------------------------------------------------- */
int lfgpu_init(int device, lfgpu_ctx** out);
int lfgpu_shutdown(lfgpu_ctx* ctx);
const char* lfgpu_last_error(const lfgpu_ctx* ctx);
int lfgpu_set_stream(lfgpu_ctx* ctx, void* hip_stream); /* NULL = default stream */
/* Gives the context a non-blocking stream of its own (destroyed by lfgpu_shutdown).  Contexts are independent -- nothing
 * below this ABI is process-global except the per-device CU budget of the resident sumcheck kernels -- so K host threads
 * may each drive one context (its circuits, provers and transcripts) on the same device concurrently; with the default
 * (NULL) stream their work would serialise.  This is the throughput mode of BM_ShaZK's loop
 * (lib/circuits/sha/flatsha256_circuit_test.cc:510-536, one proof after the other) on a GPU that one proof leaves idle. */
int lfgpu_own_stream(lfgpu_ctx* ctx);
/* RandomEngine call pattern.  The reference draws element by element (RandomEngine::elt -> Field::sample -> bytes(kBytes),
 * lib/random/random.h:38-48; one bytes(32) per Merkle nonce, lib/merkle/merkle_commitment.h:52-54).  By default the library
 * merges consecutive draws into one call of the lfgpu_rng_fn hook -- the same bytes for every engine that is a byte stream
 * (SecureRandomEngine, Transcript, the LCG test engines) and far fewer calls.  exact = 1 keeps the reference's call pattern,
 * for engines whose output depends on the call boundaries (the TestRng of rust/runtime/zk/tests/zk.rs:283-292 returns
 * {2, 0, 0, ...} for EVERY call).  Applies to lfgpu_ligero_commit and lfgpu_zk_commit on this context, and to their _batch
 * forms. */
int lfgpu_set_rng_exact_calls(lfgpu_ctx* ctx, int exact);
int lfgpu_sync(lfgpu_ctx* ctx);
/* Diagnostic, NOT part of the stable ABI: the context's pooled scratch buffer `which` (0..3; today 2 holds the Ligero-level
 * temporaries of the prove entry points): its current device address (NULL before first use) and size.  For memory accounting
 * and for the tests of the "dense block aliases the call's scratch" argument error.  The numbering, the number of buffers and
 * which entry point uses which may change in any release, and a buffer moves when it grows: nothing may be built on them. */
int lfgpu_scratch_info(const lfgpu_ctx* ctx, int which, void** d_out, size_t* bytes_out);
/* device-memory helpers so that C / ctypes / cgo callers need no HIP runtime */
int lfgpu_malloc(lfgpu_ctx* ctx, size_t bytes, void** d_out);
int lfgpu_free(lfgpu_ctx* ctx, void* d_ptr);
int lfgpu_memcpy_h2d(lfgpu_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int lfgpu_memcpy_d2h(lfgpu_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

/* ---- K1: prime-field FFT ------------------------------------------------
 * Replaces FFT<Fp128>::fftb / fftf (lib/algebra/fft.h:185-201).
 * In-place, `rows` independent length-n (power of two) transforms; row r starts
 * at d_A + r*ld.  dir 0 = backward  A[j] = sum_k A[k] w_n^{jk}, dir 1 = forward
 * (w -> w^-1); unscaled.  omega is a root of unity of order omega_order (power
 * of two >= n) in Montgomery form, exactly the (omega_j, j) arguments of fftb. */
int lfgpu_fp128_fft(lfgpu_ctx* ctx, int dir, size_t rows, size_t n, const uint64_t omega[2],
                    uint64_t omega_order, void* d_A, size_t ld);
/* Same transform over F64_2 = Fp2<Fp<1>>, p = 2^64 - 2^32 + 1 -- the second field of the reference's FFT tests and
 * benchmarks (lib/algebra/fft_test.cc:205-229, BM_FFT_F64_2).  Elements are the memory image of Fp2<Fp<1>>::Elt
 * (lib/algebra/fp2.h:48-52): {re, im}, 8 bytes each, Montgomery form (R = 2^64), reduced.  omega = {re, im} likewise;
 * a root in the base field (im = 0, as in the reference's test) takes the cheaper twiddle product. */
int lfgpu_f64_2_fft(lfgpu_ctx* ctx, int dir, size_t rows, size_t n, const uint64_t omega[2],
                    uint64_t omega_order, void* d_A, size_t ld);

/* ---- K2: additive (LCH14) FFT over GF(2^128) ------------------------------
 * Replaces LCH14<GF2_128<k>>::FFT / IFFT (lib/gf2k/lch14.h:106-144).
 * subfield_log_bits = k of GF2_128<k> (4 or 5; l <= 2^k).  dir 0 = FFT, 1 = IFFT.
 * In-place on `rows` arrays of 2^l elements, row r at d_B + r*ld. */
int lfgpu_gf2128_lch14_fft(lfgpu_ctx* ctx, int subfield_log_bits, int dir, size_t rows, unsigned l,
                           uint64_t coset, void* d_B, size_t ld);

/* ---- K3 / K4: Reed-Solomon row encode -------------------------------------
 * Replaces LCH14ReedSolomon::interpolate (lib/gf2k/lch14_reed_solomon.h:49-103)
 * and ReedSolomon::interpolate (lib/algebra/reed_solomon.h:93-110) applied to
 * every row of a tableau: y[0..n) valid -> fills y[n..m), in place, row r at
 * d_T + r*ld.  This is the InterpolatorFactory seam of LigeroProver
 * (lib/ligero/ligero_prover.h:34,175,184,210,237,295). */
int lfgpu_gf2128_rs_encode_rows(lfgpu_ctx* ctx, int subfield_log_bits, size_t nrow, size_t n, size_t m,
                                void* d_T, size_t ld);
/* The three interpolate loops of LigeroProver::commit (layout_blinding_rows / layout_witness_rows /
 * layout_quadratic_rows, lib/ligero/ligero_prover.h:171-270) in one launch: rows [lo2, hi2) hold n2 valid values,
 * every other row n1; all are extended to m.  Both lengths must fit the LDS-resident kernel (<= 4096);
 * LFGPU_ERR_UNSUPPORTED otherwise (call lfgpu_gf2128_rs_encode_rows per group instead). */
int lfgpu_gf2128_rs_encode_tableau(lfgpu_ctx* ctx, int subfield_log_bits, size_t nrow, size_t n1, size_t n2, size_t lo2,
                                   size_t hi2, size_t m, void* d_T, size_t ld);
int lfgpu_fp128_rs_encode_rows(lfgpu_ctx* ctx, size_t nrow, size_t n, size_t m, const uint64_t omega[2],
                               uint64_t omega_order, void* d_T, size_t ld);

/* The P-256 base field (BASELINE config 5, the mdoc signature circuit): replaces
 * ReedSolomon<Fp256Base, FFTExtConvolutionFactory<Fp256Base, Fp2<Fp256Base>>>::interpolate
 * (lib/algebra/reed_solomon.h:93-110 over convolution.h:129-191 / rfft.h:282-376; factory built at
 * lib/circuits/mdoc/mdoc_zk.cc:485-487) on every row of a tableau of 32-byte elements; ld counts 32-byte elements.
 * No omega argument: the interpolation does not depend on which 2^k-th root of unity carries the convolution (the
 * device uses the reference's root of order 2^31, mdoc_zk.cc:82-88). */
int lfgpu_fp256_rs_encode_rows(lfgpu_ctx* ctx, size_t nrow, size_t n, size_t m, void* d_T, size_t ld);
/* Host-buffer form: what GpuReedSolomon<Fp256Base>::interpolate (include/lfgpu_adapters.h) forwards to. */
int lfgpu_fp256_rs_encode_rows_host(lfgpu_ctx* ctx, size_t nrow, size_t n, size_t m, void* h_T, size_t ld);

/* ---- K5 + K6: Merkle column commitment ------------------------------------
 * Replaces MerkleCommitment::commit (lib/merkle/merkle_commitment.h:50-64) with
 * LigeroCommon::column_hash as updhash (lib/ligero/ligero_param.h:432-439) and
 * MerkleTree::build_tree (lib/merkle/merkle_tree.h:109-114):
 *   leaf_j = SHA256(nonce_j || ser(T[0][col0+j]) || ... || ser(T[nrow-1][col0+j]))
 *   layers[i] = SHA256(layers[2i] || layers[2i+1]),  i = ncols-1 .. 1
 * d_nonces: ncols*32 bytes (drawn by the caller from its RandomEngine in leaf
 * order, merkle_commitment.h:54).  d_layers: 2*ncols*32 bytes, heap layout of
 * MerkleTree::layers_ (leaves at [ncols, 2*ncols), root at [1]); stays on the
 * device for lfgpu_merkle_open.  root_out: 32 host bytes. */
int lfgpu_column_commit(lfgpu_ctx* ctx, int field, size_t nrow, size_t ld, size_t col0, size_t ncols,
                        const void* d_T, const void* d_nonces, void* d_layers, uint8_t root_out[32]);
/* lfgpu_column_commit for nb tableaux of one shape: leaf hash + tree of every statement in one launch each,
 * all roots in one read-back.  d_T[b], d_layers[b]: device pointers per statement (host arrays of nb pointers; the kernels
 * take them as one by-value argument, nothing is uploaded); d_nonces: [nb][ncols][32] contiguous on the device.
 * Heap b and root b are byte-identical to lfgpu_column_commit on statement b alone.  1 <= nb <= LFGPU_SC_BATCH_MAX.
 * Fields: GF2_128 and Fp128; LFGPU_ERR_UNSUPPORTED for P256 (lfgpu_column_commit_batch256 serves that field). */
int lfgpu_column_commit_batch(lfgpu_ctx* ctx, int field, size_t nrow, size_t ld, size_t col0, size_t ncols, size_t nb,
                              const void* const* d_T, const void* d_nonces, void* const* d_layers, uint8_t* roots_out /*[nb][32]*/);
/* ... for tableaux of 32-byte elements (Fp256Base): the same contract -- pointer tables by value, nonces [nb][ncols][32], heap b
 * and root b byte-identical to lfgpu_column_commit(field = LFGPU_FIELD_P256) on statement b alone, the roots in one read-back,
 * and the call's one stream synchronise at its end.  ld, col0 and ncols count 32-byte elements. */
int lfgpu_column_commit_batch256(lfgpu_ctx* ctx, size_t nrow, size_t ld, size_t col0, size_t ncols, size_t nb,
                                 const void* const* d_T, const void* d_nonces, void* const* d_layers, uint8_t* roots_out /*[nb][32]*/);
/* The leaf half of the above alone (enqueue only, nothing read back): d_leaves[j] = leaf digest of column col0 + j,
 * j < ncols, 32 bytes each.  Multi-GPU commit: after the column re-partition a rank hashes the columns it
 * owns, the digests are all-gathered into the leaf level of d_layers and lfgpu_merkle_build_tree finishes on every rank. */
int lfgpu_column_leaves(lfgpu_ctx* ctx, int field, size_t nrow, size_t ld, size_t col0, size_t ncols,
                        const void* d_T, const void* d_nonces, void* d_leaves);
/* MerkleTree::build_tree alone: d_layers[ncols..2*ncols) hold the leaves. */
int lfgpu_merkle_build_tree(lfgpu_ctx* ctx, size_t n, void* d_layers, uint8_t root_out[32]);
/* MerkleTree::generate_compressed_proof (lib/merkle/merkle_tree.h:122-143):
 * copies the sibling digests of the opening of pos[0..np) to h_path (capacity
 * path_cap digests) and writes their count to *npath. */
int lfgpu_merkle_open(lfgpu_ctx* ctx, size_t n, const void* d_layers, const size_t* pos, size_t np,
                      uint8_t* h_path, size_t path_cap, size_t* npath);

/* ---- K7 / K8 / K9: sumcheck round body -------------------------------------
 * Replaces the per-round body of ProverLayers::layer (lib/sumcheck/prover_layers.h:230-263). */
/* loop of ProverLayers::evaluations (:365-388): a0 = sum QW[2i] W[2i],
 * a2 = sum (QW[2i+1]-QW[2i]) (W[2i+1]-W[2i]) (+ odd tail).  Outputs to host. */
int lfgpu_sumcheck_partials(lfgpu_ctx* ctx, int field, size_t n, const void* d_QW, const void* d_W,
                            uint64_t a0[2], uint64_t a2[2]);
/* QW[h[hand]] += v * Wother[h[1-hand]] over the HQUAD terms (:235-243).
 * d_hc: n x {u32 h0, u32 h1}; d_vc: n elements; d_QW (nqw elements) is cleared first. */
int lfgpu_qw_scatter(lfgpu_ctx* ctx, int field, size_t n, const void* d_hc, const void* d_vc, int hand,
                     const void* d_Wother, size_t nqw, void* d_QW);
/* Dense::bind with n1 = 1 (lib/arrays/dense.h:70-87): out[i] = in[2i] + r (in[2i+1]-in[2i]);
 * d_out may equal d_in.  New length (n0+1)/2. */
int lfgpu_dense_bind(lfgpu_ctx* ctx, int field, size_t n0, const uint64_t r[2], const void* d_in,
                     void* d_out);
/* HQuad::bind_h (lib/sumcheck/hquad.h:90-123): order-preserving pairwise merge;
 * outputs to (d_hc_out, d_vc_out), *n_out = new count. */
int lfgpu_hquad_bind_h(lfgpu_ctx* ctx, int field, size_t n, const void* d_hc, const void* d_vc,
                       const uint64_t r[2], int hand, void* d_hc_out, void* d_vc_out, size_t* n_out);

/* ---- K10 / K11: sumcheck layer (Quad) resident on the device -----------------------
 * lfgpu_quad_upload: one layer's corners in EXPANDED form, in the order the reference's
 * Quad iterator yields them (canonical: Morton(h0,h1) then g, lib/sumcheck/equad.h:79-106;
 * delta decode of lib/sumcheck/quad.h:100-130 done by the caller), vi indexing the shared
 * constant table kvec (nk elements; a zero constant marks an assert-zero term, quad.h:213-220).
 * nv = number of output gates of the layer.  Upload once per circuit; reuse per proof. */
typedef struct lfgpu_quad lfgpu_quad;
int lfgpu_quad_upload(lfgpu_ctx* ctx, int field, size_t nterms, const uint32_t* g, const uint32_t* h0,
                      const uint32_t* h1, const uint32_t* vi, size_t nk, const void* h_kvec, size_t nv,
                      lfgpu_quad** out);
int lfgpu_quad_free(lfgpu_quad* q);
/* ProverLayers::eval_quad with nc = 1 (lib/sumcheck/prover_layers.h:278-305):
 * V[g] = sum kvec[vi] * W[h1] * W[h0]; *ok = 0 if an assert-zero term is non-zero
 * (the reference returns false / eval_circuit returns nullptr). */
int lfgpu_eval_quad(lfgpu_quad* q, size_t nw, const void* d_W, void* d_V, int* ok);
/* Quad::bind_g (lib/sumcheck/quad.h:152-185): HQUAD[(h0,h1)] = sum_g prep_v(v, beta) *
 * (EQ(G0,g) + alpha EQ(G1,g)); outputs the compact HQuad (d_hc_out: pairs of u32, d_vc_out:
 * elements; capacity nterms) and its size. */
int lfgpu_quad_bind_g(lfgpu_quad* q, size_t logv, const void* h_G0, const void* h_G1, const uint64_t alpha[2],
                      const uint64_t beta[2], void* d_hc_out, void* d_vc_out, size_t* n_out);

/* Eqs::raw_eq2 (lib/arrays/eqs.h): eq[i] = EQ(G0, i) + alpha EQ(G1, i) for i < n <= 2^logn, the
 * vector bind_g folds the corners with and ZkCommon::input_constraint (lib/zk/zk_common.h:406-439) puts on the
 * inputs.  h_G0 / h_G1: logn host elements; d_eq: n device elements. */
int lfgpu_raw_eq2(lfgpu_ctx* ctx, int field, size_t logn, size_t n, const void* h_G0, const void* h_G1,
                  const uint64_t alpha[2], void* d_eq);

/* Quad::bind_gh_all (lib/sumcheck/quad.h:188-210), the verifier's combined bind_g + bind_h:
 * out = sum over the corners of prep_v(v, beta) (EQ(G0,g) + alpha EQ(G1,g)) EQ(H0,h0) EQ(H1,h1).
 * nw = number of input wires of the layer (hand indices are < nw <= 2^logw). */
int lfgpu_quad_bind_gh_all(lfgpu_quad* q, size_t logv, const void* h_G0, const void* h_G1, const uint64_t alpha[2],
                           const uint64_t beta[2], size_t logw, size_t nw, const void* h_H0, const void* h_H1,
                           uint64_t out[2]);

/* ---- one whole sumcheck layer with the transcript behind a callback -------------------
 * Replaces the body of ProverLayers::layer for logc = 0 (every ZK use, lib/zk/zk_common.h:72) together
 * with the bind_g that precedes it (lib/sumcheck/prover_layers.h:140-146,185-271): HQUAD = bind_g(...),
 * then for round < logw, hand in {0,1}: QW scatter, evaluations() -> the 3 evaluations of the round
 * polynomial at poly_evaluation_point(0..2), `round` callback (the caller's round_h: subtract pad, store in
 * the proof, ts.round(poly) -> challenge), bind W[hand] and HQUAD.  The Fiat-Shamir transcript never
 * leaves the caller.  d_W: the layer's nw input wires (device; consumed).  wc_in: the two claims of the
 * previous layer; outputs: wc_out = W[R,C], W[L,C]; g_out[hand][round] = the challenges (next layer's
 * G0/G1); bound_quad = HQUAD->scalar() (ProofAux::bound_quad). */
typedef void (*lfgpu_sc_round_fn)(void* user, size_t hand, size_t round, const uint64_t evals[3][2],
                                  uint64_t challenge_out[2]);
int lfgpu_sumcheck_layer(lfgpu_quad* q, size_t logv, const void* h_G0, const void* h_G1, const uint64_t alpha[2],
                         const uint64_t beta[2], size_t logw, size_t nw, void* d_W, const uint64_t wc_in[2][2],
                         lfgpu_sc_round_fn round, void* user, uint64_t wc_out[2][2], uint64_t* g_out /*[2][logw][2]*/,
                         uint64_t bound_quad[2]);

/* ---- the same layer for a batch of statements in lock-step (K14) -------------------------------------
 * nb statements of ONE quad (one circuit layer, nb witnesses) go through the same launches: bind_g of all statements in at
 * most three, then every round-hand of all statements in a number of launches that does not depend on nb, with ONE host round trip -- one call of
 * `round` -- per round-hand.  Statement b's evaluations, wc_out, g_out and bound_quad are byte-identical to what
 * lfgpu_sumcheck_layer produces for statement b alone when its callback returns the same challenges.
 * `round` is called 2 * logw times, in the order (round 0, hand 0), (round 0, hand 1), (round 1, hand 0), ...: evals[b] = the
 * 3 evaluations of statement b's round polynomial, challenge_out[b] = its challenge.
 * h_G0 / h_G1: [nb][logv] host elements, statement b at offset b * logv; alpha, beta: [nb][2]; d_W: statement b's nw wires at
 * d_W + b * ldw elements, ldw >= nw (device; consumed); wc_in: [nb][2][2]; wc_out: [nb][2][2]; g_out: [nb][2][logw][2];
 * bound_quad: [nb][2] or NULL.  1 <= nb <= LFGPU_SC_BATCH_MAX (the challenges of a round-hand are then 1 KiB of kernel
 * arguments and the mailbox 8 KiB: a condition of the design, not a tuned number).  Fields: GF2_128 and Fp128;
 * LFGPU_ERR_UNSUPPORTED for P256.  The driver launches one kernel chain per round-hand and no resident kernel: the
 * LFGPU_SC_* switches of lfgpu_sumcheck_layer have no effect on it. */
#define LFGPU_SC_BATCH_MAX 64
typedef void (*lfgpu_sc_round_batch_fn)(void* user, size_t hand, size_t round, size_t nb, const uint64_t (*evals)[3][2],
                                        uint64_t (*challenge_out)[2]);
int lfgpu_sumcheck_layer_batch(lfgpu_quad* q, size_t nb, size_t logv, const void* h_G0, const void* h_G1, const uint64_t* alpha,
                               const uint64_t* beta, size_t logw, size_t nw, void* d_W, size_t ldw, const uint64_t* wc_in,
                               lfgpu_sc_round_batch_fn round, void* user, uint64_t* wc_out, uint64_t* g_out,
                               uint64_t* bound_quad);
/* ProverLayers::eval_quad (nc = 1) for nb statements of ONE quad in one launch: statement b reads its nw wires at
 * d_W + b * ldw elements (ldw >= nw) and writes its nv outputs at d_V + b * ldv elements (ldv >= nv); ok_out[b] = 0 if an
 * assert-zero term of statement b is non-zero, the other statements are unaffected.  1 <= nb <= LFGPU_SC_BATCH_MAX.
 * Fields: GF2_128 and Fp128; LFGPU_ERR_UNSUPPORTED for P256. */
int lfgpu_eval_quad_batch(lfgpu_quad* q, size_t nb, size_t nw, const void* d_W, size_t ldw, void* d_V, size_t ldv,
                          int* ok_out /*[nb]*/);

/* ---- the sumcheck layer over Fp256Base (field 1), single and in lock-step -------------------------------
 * Elements are 4 x u64 LE Montgomery images (R = 2^256), canonical (< p); ld / strides count 32-byte elements.  These take
 * quads of LFGPU_FIELD_P256 only (LFGPU_ERR_ARG for a quad of a 16-byte field), as the entry points above take the 16-byte
 * fields only.  All argument errors are found on the host before the first launch: LFGPU_ERR_ARG for a NULL argument, nb
 * outside 1..LFGPU_SC_BATCH_MAX, ldw < nw, nw <= the largest hand index, 2^logv < nv, ldv < nv; LFGPU_ERR_NOMEM when the
 * per-statement scratch does not fit (the limb accumulators alone are 64 bytes per entry and statement).  A NULL quad returns
 * LFGPU_ERR_ARG without a context.
 *
 * lfgpu_sumcheck_layer256: lfgpu_sumcheck_layer for Fp256Base -- the layer lfgpu_zk_prove runs, with all its modes (the
 * resident grid, the per-launch kernels, the LFGPU_P256_* switches).  h_G0 / h_G1: logv host elements.  Unlike the 16-byte
 * call, d_W is LEFT INTACT: both hands bind into buffers of the context. */
typedef void (*lfgpu_sc_round256_fn)(void* user, size_t hand, size_t round, const uint64_t evals[3][4],
                                     uint64_t challenge_out[4]);
int lfgpu_sumcheck_layer256(lfgpu_quad* q, size_t logv, const void* h_G0, const void* h_G1, const uint64_t alpha[4],
                            const uint64_t beta[4], size_t logw, size_t nw, const void* d_W, const uint64_t wc_in[2][4],
                            lfgpu_sc_round256_fn round, void* user, uint64_t wc_out[2][4],
                            uint64_t* g_out /*[2][logw][4]*/, uint64_t bound_quad[4]);
/* lfgpu_sumcheck_layer_batch (K14) for Fp256Base: nb statements of ONE quad through the same launches, ONE call of `round` per
 * round-hand for all statements, in the order (round 0, hand 0), (round 0, hand 1), (round 1, hand 0), ...  Statement b's
 * evaluations, wc_out, g_out and bound_quad are byte-identical to what lfgpu_sumcheck_layer256 gives for statement b alone
 * under the same challenges.  h_G0 / h_G1: [nb][logv]; alpha, beta: [nb][4]; d_W: statement b's nw wires at d_W + b * ldw
 * elements, ldw >= nw (device; NOT modified, its padding included); wc_in, wc_out: [nb][2][4]; g_out: [nb][2][logw][4];
 * bound_quad: [nb][4] or NULL.  1 <= nb <= LFGPU_SC_BATCH_MAX (the challenges of a round-hand are then 2 KiB of kernel
 * arguments).  The challenges the callback returns must be canonical (a precondition, not checked).
 * No resident grid: while the HQUAD or a hand array has more than LFGPU_P256_BATCH_SMALL_MAX entries a round-hand is three
 * launches whatever nb; from then on it is one launch of nb workgroups that keeps a statement's accumulators in LDS.
 * LFGPU_P256_BATCH_SMALL=0 (environment, read once per process) keeps the three launches throughout: the same bytes. */
#define LFGPU_P256_BATCH_SMALL_MAX 2048
typedef void (*lfgpu_sc_round_batch256_fn)(void* user, size_t hand, size_t round, size_t nb, const uint64_t (*evals)[3][4],
                                           uint64_t (*challenge_out)[4]);
int lfgpu_sumcheck_layer_batch256(lfgpu_quad* q, size_t nb, size_t logv, const void* h_G0, const void* h_G1,
                                  const uint64_t* alpha, const uint64_t* beta, size_t logw, size_t nw, const void* d_W,
                                  size_t ldw, const uint64_t* wc_in, lfgpu_sc_round_batch256_fn round, void* user,
                                  uint64_t* wc_out, uint64_t* g_out, uint64_t* bound_quad /* may be NULL */);
/* lfgpu_eval_quad_batch for Fp256Base: statement b reads its nw wires at d_W + b * ldw (ldw >= nw), writes its nv outputs at
 * d_V + b * ldv (ldv >= nv); ok_out[b] = 0 only for the statements whose assert-zero terms fail, the others are unaffected. */
int lfgpu_eval_quad_batch256(lfgpu_quad* q, size_t nb, size_t nw, const void* d_W, size_t ldw, void* d_V, size_t ldv,
                             int* ok_out /*[nb]*/);

/* ---- circuits with nc > 1 copies: the copy rounds of the sumcheck (K13) ------------------------------
 * The reference's data-parallel axis: every wire array is Dense(n0 = nc, n1 = nw), stored W[wire * nc + c] (copy index
 * fastest, lib/arrays/dense.h:44-45), and every layer opens with logc cubic rounds that bind the copy variable
 * (lib/sumcheck/prover_layers.h:196-216) before the hand rounds above.  Fields: GF2_128 and Fp128; LFGPU_ERR_UNSUPPORTED for
 * P256.  The prover-level ABI of lfgpu_zk.h stays at nc = 1, as the reference's ZkProver does (lib/zk/zk_common.h:72). */
/* ProverLayers::eval_quad over all copies (lib/sumcheck/prover_layers.h:278-305): V[g * nc + c] = sum kvec[vi] *
 * W[h1 * nc + c] * W[h0 * nc + c]; the assert-zero terms are checked in every copy, *ok = 0 if any copy fails.
 * d_W: nw * nc elements, d_V: nv * nc elements. */
int lfgpu_eval_quad_copies(lfgpu_quad* q, size_t nc, size_t nw, const void* d_W, void* d_V, int* ok);
/* The loop of ProverLayers::evaluations_c (lib/sumcheck/prover_layers.h:418-477, odd tail :460-472) and the three
 * F.reduce of :480-482: acc_out[0], [1], [2] = the coefficients coefs[0], coefs[2], coefs[3] of the round's cubic.
 * d_hc / d_vc: the nh HQUAD terms (as lfgpu_quad_bind_g leaves them); d_W: [nrows][n0];
 * d_eq: the current EQ vector, n0 elements.  Outputs to host.  nrows states the shape of d_W and is checked only for 0:
 * the hand indices live on the device and are NOT validated, so the caller guarantees that every one is < nrows (an
 * index past it reads outside d_W). */
int lfgpu_sumcheck_evaluations_c(lfgpu_ctx* ctx, int field, size_t nh, const void* d_hc, const void* d_vc, size_t n0,
                                 size_t nrows, const void* d_W, const void* d_eq, uint64_t acc_out[3][2]);
/* Dense::bind with n1 = nrows (lib/arrays/dense.h:70-87): out[i1][i] = in[i1][2i] + r (in[i1][2i+1] - in[i1][2i]), the
 * rows re-packed to stride (n0 + 1) / 2 (:74-85).  Out of place only (the compaction makes a parallel bind in place a
 * race): LFGPU_ERR_ARG if the two buffers overlap. */
int lfgpu_dense_bind_rows(lfgpu_ctx* ctx, int field, size_t n0, size_t nrows, const uint64_t r[2], const void* d_in,
                          void* d_out);
/* Eqs::filleq, i.e. the Eqs(logn, n, Q) constructor (lib/arrays/eqs.h:36-39,104-134): eq[i] = EQ(Q, i), i < n <= 2^logn.
 * h_Q: logn host elements; d_eq: n device elements.  Eqs::bind is Dense::bind: lfgpu_dense_bind. */
int lfgpu_eqs(lfgpu_ctx* ctx, int field, size_t logn, size_t n, const void* h_Q, void* d_eq);
/* The whole of ProverLayers::layer (lib/sumcheck/prover_layers.h:185-271) with the Eqs constructor and the bind_g in
 * front of it (:155-157): lfgpu_sumcheck_layer plus the copy rounds.  For round < logc: evaluations_c -> the 4 evaluations
 * of the round's cubic at poly_evaluation_point(0..3) -> `round_c` callback (the caller's round_c, :307-318: subtract pad,
 * store in the proof, ts.round(poly) -> challenge) -> bind EQ and W.  Then eq0 = EQ->scalar() and the hand rounds of
 * lfgpu_sumcheck_layer run on the [nw] vector that is left, their coefficients scaled by eq0.  d_W: [nw][nc] (device;
 * consumed); h_Q: logc host elements (the previous layer's q_out); q_out[round] = the copy challenges (bnd.q, the next
 * layer's Q); the other arguments as for lfgpu_sumcheck_layer.  0 < nc <= 2^logc <= 2^40; logc = 0, nc = 1 is
 * lfgpu_sumcheck_layer (h_Q, round_c and q_out may then be NULL). */
typedef void (*lfgpu_sc_round_c_fn)(void* user, size_t round, const uint64_t evals[4][2], uint64_t challenge_out[2]);
int lfgpu_sumcheck_layer_copies(lfgpu_quad* q, size_t logc, size_t nc, const void* h_Q, size_t logv, const void* h_G0,
                                const void* h_G1, const uint64_t alpha[2], const uint64_t beta[2], size_t logw, size_t nw,
                                void* d_W, const uint64_t wc_in[2][2], lfgpu_sc_round_c_fn round_c, lfgpu_sc_round_fn round_h,
                                void* user, uint64_t wc_out[2][2], uint64_t* q_out /*[logc][2]*/,
                                uint64_t* g_out /*[2][logw][2]*/, uint64_t bound_quad[2]);

/* ---- element-wise field ops (Field::addf / subf / mulf, lib/gf2k/gf2_128.h:227-237,
 * lib/algebra/fp_generic.h:203-214): out[i] = a[i] op b[i], op 0 add, 1 sub, 2 mul.  Used by the
 * parity tests to pin the device arithmetic directly. */
int lfgpu_field_binop(lfgpu_ctx* ctx, int field, int op, size_t n, const void* d_a, const void* d_b, void* d_out);

/* ---- K12: Ligero row combinations -----------------------------------------
 * y[j] += sum_i u[i] * T[i][j], j < n  (low_degree_proof, lib/ligero/ligero_prover.h:281-291;
 * Blas::axpy lib/algebra/blas.h:62-68).  h_u: nrows host elements. */
int lfgpu_rows_axpy(lfgpu_ctx* ctx, int field, size_t nrows, size_t n, void* d_y, const uint64_t* h_u,
                    const void* d_T, size_t ld);
/* req[i][j] = T[i][col0 + idx[j]]  (compute_req :346-351; Blas::gather blas.h:104-110) */
int lfgpu_gather_columns(lfgpu_ctx* ctx, size_t nrow, size_t ld, size_t col0, const void* d_T,
                         const size_t* h_idx, size_t nreq, void* d_req);

/* ---- Ligero commit / prove on a device-resident tableau -----------------------
 * The device boundary the survey recommends: inside LigeroProver::commit the witness is
 * uploaded once, the tableau [nrow][block_enc] stays in HBM, and only the root (and later
 * y_ldt / y_dot / y_quad / req) come back.  The Fiat-Shamir transcript and the
 * RandomEngine stay with the caller: randomness is drawn through `rng` in exactly the
 * reference's order (lib/ligero/ligero_prover.h:171-270, lib/merkle/merkle_commitment.h:54). */
typedef struct {
  /* LigeroParam (lib/ligero/ligero_param.h:117-307) */
  size_t nw, nq, rateinv, nreq;
  size_t block_enc, block, dblock, block_ext, r, w, nwrow, nqtriples, nwqrow, nrow, mc_pathlen;
  size_t ildt, idot, iquad, iw, iq;
} lfgpu_ligero_param;
/* LigeroParam(nw, nq, rateinv, nreq, block_enc) ctor (block_enc = 0: the deprecated ctor that searches
 * block_enc over powers of two for the smallest proof, ligero_param.h:152-169); LFGPU_ERR_ARG where the reference
 * would check-fail ("block_enc too large").  field selects kSubFieldBytes (GF2_128<k>: 2^k/8). */
int lfgpu_ligero_param_init(lfgpu_ligero_param* p, int field, int subfield_log_bits, size_t nw, size_t nq,
                            size_t rateinv, size_t nreq, size_t block_enc);
/* RandomEngine::bytes (lib/random/random.h:32-35) */
typedef void (*lfgpu_rng_fn)(void* user, uint8_t* buf, size_t n);
typedef struct lfgpu_ligero_prover lfgpu_ligero_prover;
/* LigeroProver::commit (lib/ligero/ligero_prover.h:58-79) minus the transcript write:
 * layout (blinding / witness / quadratic rows), RS-encode every row, Merkle-commit the
 * columns [dblock, block_enc).  h_W: nw host elements; h_lqc: nq x {x,y,z}.  GF2_128: every h_W[i], i < subfield_boundary,
 * must lie in the subfield (the reference's check, :63-66; such rows are blinded with subfield randomness): LFGPU_ERR_ARG with
 * the index in the message otherwise, before anything is drawn from rng.  The same holds for every entry point below that
 * lays out witness rows (commit_batch, layout_rows, layout_rows_sharded, commit_sharded).
 * Fields: GF2_128, Fp128 and P256 (h_W: 32-byte Montgomery elements; the returned prover serves low_degree_proof, dot_proof,
 * quadratic_proof, open, tableau, free and lfgpu_ligero_prove256, and is refused by every other entry point that takes one). */
int lfgpu_ligero_commit(lfgpu_ctx* ctx, int field, int subfield_log_bits, const lfgpu_ligero_param* p,
                        const void* h_W, size_t subfield_boundary, const size_t* h_lqc, lfgpu_rng_fn rng,
                        void* rng_user, uint8_t root_out[32], lfgpu_ligero_prover** out);
/* nb x lfgpu_ligero_commit of ONE lfgpu_ligero_param and one h_lqc, each statement with its own witness and RandomEngine.
 * The host layout runs per statement in index order b = 0 .. nb-1, every draw of statement b from rng[b] (user rng_user[b];
 * rng_user = NULL: every user is NULL) in lfgpu_ligero_commit's order, lfgpu_set_rng_exact_calls honoured.  Handing the SAME
 * engine to several statements therefore gives the bytes of sequential lfgpu_ligero_commit calls in index order.  The device
 * half is one chain for all statements: asynchronous uploads from pinned staging memory (kept by the context for the next
 * call, scrubbed after each), the Reed-Solomon encode with the statement on a grid axis, one leaf-hash launch, the Merkle
 * levels with the statement on a grid axis, all roots in one read-back and ONE stream synchronise.  GF(2^128) rows longer
 * than 2^12 (the shapes lfgpu_gf2128_rs_encode_tableau refuses) are encoded per statement with lfgpu_ligero_commit's own
 * encoder inside the call: correct, merely unbatched.  Fp128: the statements are chunked so that a launch holds at most
 * 65535 rows and the convolution scratch stays under 256 MiB (LFGPU_CB_CHUNK=<statements per chain> overrides, read once).
 * Roots, tableaux, Merkle heaps and nonces are byte-identical to nb lfgpu_ligero_commit calls; each out[b] is an ordinary
 * prover that owns its pooled buffers (every prove / open / free entry point works on it; free in any order).
 * LFGPU_COMMIT_BATCH=0 (read once) keeps these semantics and runs the single-statement device path per statement.
 * 1 <= nb <= LFGPU_SC_BATCH_MAX, else LFGPU_ERR_ARG; argument errors are found before the first draw.  An error inside
 * statement b's layout (LFGPU_ERR_ARG: lqc index out of range, or a witness below subfield_boundary outside the subfield; LFGPU_ERR_ASSERT: a quadratic constraint does not hold) fails
 * the whole call: out[0 .. nb) are NULL and every buffer is back in the pool, scrubbed.  Fields: GF2_128 and Fp128. */
int lfgpu_ligero_commit_batch(lfgpu_ctx* ctx, int field, int subfield_log_bits, const lfgpu_ligero_param* p, size_t nb,
                              const void* const* h_W, size_t subfield_boundary, const size_t* h_lqc,
                              const lfgpu_rng_fn* rng, void* const* rng_user, uint8_t* roots_out /*[nb][32]*/,
                              lfgpu_ligero_prover** out /*[nb]*/);
/* lfgpu_ligero_commit_batch over Fp256Base: nb x lfgpu_ligero_commit(field = LFGPU_FIELD_P256) of ONE lfgpu_ligero_param and one
 * h_lqc (h_W[b]: nw 32-byte Montgomery elements).  The contract is the one above: the host layout per statement in index order,
 * every draw of statement b from rng[b] in lfgpu_ligero_commit's order with lfgpu_set_rng_exact_calls honoured, so one engine
 * handed to several statements sees the draw order of sequential calls; pinned staging kept by the context and scrubbed after
 * every call; ONE stream synchronise; on any error out[0 .. nb) are NULL, and the stream is synchronised before the staging is
 * scrubbed.  The device half per chain of statements: the rows that carry `block` values ([0, IDOT) and (IQUAD, nrow)) of ALL
 * statements go through one convolution, the IDOT / IQUAD rows of all statements through a second -- two rows share one complex
 * transform, across statements too (exact arithmetic: the pairing does not change a byte) -- then one leaf-hash launch and the
 * Merkle levels with the statement on a grid axis (lfgpu_column_commit_batch256).  The encoder's tables of both shapes are made
 * sure of before anything is enqueued, so a warm call does not synchronise in the middle.  Statements are chunked so that a
 * chain's row pairs fit one launch (65535) and its convolution scratch (64 bytes per point) stays under 256 MiB;
 * LFGPU_CB_CHUNK overrides as above.  A shape of which not even one statement fits is encoded per statement with
 * lfgpu_ligero_commit's own encoder inside the call; block_enc above 2^24 is LFGPU_ERR_UNSUPPORTED, as in lfgpu_ligero_commit.
 * Roots, tableaux, Merkle heaps and nonces are byte-identical to nb lfgpu_ligero_commit calls; each out[b] is a prover of the kind
 * lfgpu_ligero_commit(field = LFGPU_FIELD_P256) returns (low_degree_proof, dot_proof, quadratic_proof, open, tableau, free,
 * lfgpu_ligero_prove256, lfgpu_ligero_prove_batch256, lfgpu_ligero_open_batch256).  LFGPU_COMMIT_BATCH256=0 (read once per
 * process) keeps these semantics and runs the single-statement device path per statement: the same bytes.
 * 1 <= nb <= LFGPU_SC_BATCH_MAX, else LFGPU_ERR_ARG; argument errors are found before the first draw. */
int lfgpu_ligero_commit_batch256(lfgpu_ctx* ctx, const lfgpu_ligero_param* p, size_t nb, const void* const* h_W,
                                 const size_t* h_lqc, const lfgpu_rng_fn* rng, void* const* rng_user,
                                 uint8_t* roots_out /*[nb][32]*/, lfgpu_ligero_prover** out /*[nb]*/);
/* LigeroProver::commit split for a row slab [row_lo, row_hi) of the tableau -- the multi-GPU form (rows are independent
 * up to the RandomEngine's draw order, lib/ligero/ligero_prover.h:171-270).
 *  lfgpu_ligero_layout_rows: HOST ONLY (no context, no device).  Performs every RandomEngine draw of commit in the
 *    reference's order -- blinding rows, witness-row pads, quadratic-row pads, then the block_ext Merkle nonces -- and
 *    writes the un-encoded image of the slab's rows to h_rows [(row_hi-row_lo)][dblock] (rows outside the slab are drawn
 *    and dropped).  Ranks that are handed the same byte stream (one engine's output broadcast, or one seed) therefore hold
 *    consistent slabs of one tableau.  h_nonces: block_ext * 32 bytes, or NULL.
 *  lfgpu_ligero_encode_rows: uploads h_rows and RS-extends each row to block_enc into d_slab [(row_hi-row_lo)][block_enc]
 *    (rows IDOT / IQUAD carry dblock values, the others block).
 * lfgpu_ligero_commit is exactly layout_rows + encode_rows on [0, nrow) followed by lfgpu_column_commit.
 * layout_rows takes all three fields (P256: h_W and h_rows hold 32-byte elements); encode_rows the two 16-byte fields (for P256
 * the rows go through lfgpu_fp256_rs_encode_rows: block values for every row but IDOT / IQUAD, which carry dblock). */
int lfgpu_ligero_layout_rows(int field, int subfield_log_bits, const lfgpu_ligero_param* p, const void* h_W,
                             size_t subfield_boundary, const size_t* h_lqc, lfgpu_rng_fn rng, void* rng_user,
                             size_t row_lo, size_t row_hi, void* h_rows, uint8_t* h_nonces);
int lfgpu_ligero_encode_rows(lfgpu_ctx* ctx, int field, int subfield_log_bits, const lfgpu_ligero_param* p,
                             size_t row_lo, size_t row_hi, const void* h_rows, void* d_slab);
/* A prover object over a slab that was laid out and encoded with the two calls above (not owning d_slab / d_layers).
 * The prove entry points below then return the slab's PARTIAL results: rows the slab does not hold contribute zero to
 * y_ldt / y_dot / y_quad (the caller folds the ranks' vectors with the field's addition and checks the W part of y_quad),
 * lfgpu_ligero_open returns the slab's rows of req.  The quadratic rows [iq, nrow) must lie in ONE slab (a triple is
 * multiplied element-wise).  d_layers (whole heap, 2*block_ext*32 bytes) and h_nonces (block_ext*32) are only needed for
 * lfgpu_ligero_open and may be NULL. */
int lfgpu_ligero_prover_from_slab(lfgpu_ctx* ctx, int field, int subfield_log_bits, const lfgpu_ligero_param* p,
                                  size_t row_lo, size_t row_hi, void* d_slab, void* d_layers, const uint8_t* h_nonces,
                                  lfgpu_ligero_prover** out);
/* ---- LigeroProver with the tableau rows sharded over the GPUs of a node, behind this ABI -------------------------
 * One process per GPU; every rank calls the same entry points with the same arguments (SPMD).  The library does the
 * orchestration -- RandomEngine stream drawn once on rank 0 and replayed everywhere, row-slab RS encode (no collective),
 * ONE all_to_all that re-partitions the encoded columns, local column hash, all_gather of the leaf digests, the tree on every
 * rank; the prove entry points below fold the ranks' partial vectors with the FIELD's addition -- and reaches the transport
 * through three hooks, the way the transcript and the RandomEngine are hooks: the caller binds them to RCCL (one
 * ncclAllGather / grouped ncclSend+ncclRecv / ncclBroadcast each; longfellow-zk_amd/parallel.py binds torch.distributed).
 * Buffers are raw bytes; on_device = 1: device memory, and the exchange must be ordered after the work already enqueued on
 * `stream` (the context's stream) and be complete, or enqueued on that stream, when the hook returns; on_device = 0: host.
 * Every hook returns 0 on success.  Results (root, y vectors, opened columns, Merkle path) are identical on every rank and
 * identical to the one-GPU lfgpu_ligero_commit fed the same RandomEngine. */
typedef struct lfgpu_comm_ops {
  void* user;
  int rank, world;
  /* every rank contributes `bytes` bytes; recv gets world * bytes, in rank order */
  int (*all_gather)(void* user, const void* send, void* recv, size_t bytes, int on_device, void* stream);
  /* rank q receives, from every rank p, the send_bytes[q] bytes at send + send_off[q] of p, into recv + recv_off[p]
   * (recv_bytes[p] = what p sends to this rank); the arrays have `world` entries */
  int (*all_to_all)(void* user, const void* send, const size_t* send_off, const size_t* send_bytes, void* recv,
                    const size_t* recv_off, const size_t* recv_bytes, int on_device, void* stream);
  int (*broadcast)(void* user, void* buf, size_t bytes, int root, int on_device, void* stream);
} lfgpu_comm_ops;
/* row slab [*row_lo, *row_hi) of rank `rank`: an even split of the rows, except that the quadratic rows [iq, nrow) all go to
 * the last rank (a triple x, y, z is multiplied element-wise) */
int lfgpu_ligero_row_shard(const lfgpu_ligero_param* p, int rank, int world, size_t* row_lo, size_t* row_hi);
/* The host half alone (no device): rank 0 performs every RandomEngine draw of LigeroProver::commit once (`rng` is only
 * called there), the byte stream is broadcast, and every rank lays out its slab from it (as lfgpu_ligero_layout_rows). */
int lfgpu_ligero_layout_rows_sharded(int field, int subfield_log_bits, const lfgpu_ligero_param* p, const void* h_W,
                                     size_t subfield_boundary, const size_t* h_lqc, lfgpu_rng_fn rng, void* rng_user,
                                     const lfgpu_comm_ops* comm, void* h_rows, uint8_t* h_nonces);
/* LigeroProver::commit (lib/ligero/ligero_prover.h:58-79) over comm->world GPUs.  The prover object it returns is used with
 * the SAME prove entry points as a one-GPU prover (low_degree_proof, dot_proof[_sparse], quadratic_proof, open): they return
 * the complete vectors on every rank. */
int lfgpu_ligero_commit_sharded(lfgpu_ctx* ctx, int field, int subfield_log_bits, const lfgpu_ligero_param* p,
                                const void* h_W, size_t subfield_boundary, const size_t* h_lqc, lfgpu_rng_fn rng,
                                void* rng_user, const lfgpu_comm_ops* comm, uint8_t root_out[32], lfgpu_ligero_prover** out);
/* host-only self-test of a caller's hooks (each with host buffers, world > 1 or 1): 0 when all three move the right bytes */
int lfgpu_comm_selftest(const lfgpu_comm_ops* comm);
/* low_degree_proof (:281-291): y[block] = T[ildt] + sum_i u_ldt[i] T[iw+i] */
int lfgpu_ligero_low_degree_proof(lfgpu_ligero_prover* pr, const void* h_u_ldt, void* h_y);
/* dot_proof (:293-309): y[dblock] = T[idot] + sum_i RS(block->dblock)([0^r | A_i]) (.) T[iw+i]; h_A: nwqrow x w host elements.
 * This one, low_degree_proof, quadratic_proof and open take a prover of any of the three fields. */
int lfgpu_ligero_dot_proof(lfgpu_ligero_prover* pr, const void* h_A, void* h_y);
/* The same with the matrix A built on the device (inner_product_vector + layout_Aext, ligero_param.h:382-430):
 *   A[t] = scale * d_dense[t] for t < ndense  (the private-input block of the last constraint: d_dense is the
 *          device-resident EQ table of lfgpu_raw_eq2 past the public inputs, scale its alphal),
 *   A[h_idx[t]] += h_val[t] for the nsparse remaining terms (host side: strictly increasing flat indices, duplicates
 *          folded by the caller).
 * lfgpu_ligero_inner_product_rows writes the rows [0^r | A_i] at stride ld into d_rows (nrows rows; the first r + w
 * columns of every row are cleared first) -- what LigeroVerifier extends and compares (ligero_verifier.h:150-190). */
int lfgpu_ligero_inner_product_rows(lfgpu_ctx* ctx, int field, size_t w, size_t r, size_t ld, size_t nrows, const void* d_dense,
                                    size_t ndense, const uint64_t scale[2], const uint64_t* h_idx, const void* h_val,
                                    size_t nsparse, void* d_rows);
/* (16-byte fields; a P-256 prover: LFGPU_ERR_ARG) */
int lfgpu_ligero_dot_proof_sparse(lfgpu_ligero_prover* pr, const void* d_dense, size_t ndense, const uint64_t scale[2],
                                  const uint64_t* h_idx, const void* h_val, size_t nsparse, void* h_y);
/* quadratic_proof (:311-344); LFGPU_ERR_ASSERT if the W part of y is non-zero */
int lfgpu_ligero_quadratic_proof(lfgpu_ligero_prover* pr, const void* h_u_quad, void* h_y0, void* h_y2);
/* compute_req (:346-351) + MerkleCommitment::open (merkle_commitment.h:66-73) */
int lfgpu_ligero_open(lfgpu_ligero_prover* pr, const size_t* idx, void* h_req, uint8_t* h_nonces,
                      uint8_t* h_path, size_t path_cap, size_t* npath);
/* ---- LigeroProver::prove for nb committed provers of ONE context, field (GF2_128 or Fp128) and lfgpu_ligero_param ----
 * lfgpu_ligero_prove_batch: the low-degree, dot (sparse form) and quadratic proofs of all statements in one chain of
 * dispatches with the statement on a grid axis -- one memset, one dense and one sparse launch for the A rows of all
 * statements, their Reed-Solomon extension, the dot-proof, low-degree and quadratic combinations (one launch each) -- and one
 * read-back.  Statement b's arguments are what the three single calls
 * take: h_u_ldt [nb][nwqrow], d_dense[b] (device; ndense elements, the same count for every statement; may hold NULLs when
 * ndense == 0) with scale [nb][2], the sparse list h_idx[b] / h_val[b] of nsparse[b] entries (0 allowed; strictly
 * increasing flat indices below nwqrow * w), h_u_quad [nb][nqtriples] (NULL when nqtriples == 0).  Outputs: h_y_ldt
 * [nb][block], h_y_dot [nb][dblock], h_y_q0 [nb][r], h_y_q2 [nb][dblock - block], byte-identical to
 * lfgpu_ligero_low_degree_proof, lfgpu_ligero_dot_proof_sparse and lfgpu_ligero_quadratic_proof on pr[b] alone.
 * lfgpu_ligero_open_batch: lfgpu_ligero_open for all statements -- one column gather, one digest gather, one read-back.
 * idx: [nb][nreq]; h_req [nb][nrow][nreq]; h_nonces [nb][nreq][32]; statement b's npath[b] path digests at
 * h_path + b * path_cap * 32 (the lengths differ with the opened positions).
 * Working memory comes from the context's pooled scratch (it grows on the first call at a shape; later calls allocate
 * nothing).  It holds the A rows (public), the y vectors and the opened columns (proof bytes) and challenge vectors: nothing
 * of it is scrubbed.  Statements are chunked so that a chain's working set and its Fp128 convolution scratch stay under
 * 256 MiB and the rows of a chain's Fp128 extension fit one launch; LFGPU_LP_CHUNK=<statements per chain> overrides (read once).
 * 1 <= nb <= LFGPU_SC_BATCH_MAX.  LFGPU_ERR_ARG, found before anything is enqueued or written: a NULL entry, a prover of
 * another context, field or lfgpu_ligero_param, the same prover twice, a sparse list that is not strictly increasing or out of
 * range, an opened index out of range or given twice within a statement, a dense block inside the call's scratch.
 * LFGPU_ERR_UNSUPPORTED: a sharded prover or a slab prover (row_lo != 0 || row_hi != nrow), Fp256Base.  LFGPU_ERR_ASSERT: the
 * W part of a statement's y_quad is non-zero (as lfgpu_ligero_quadratic_proof). */
int lfgpu_ligero_prove_batch(lfgpu_ctx* ctx, lfgpu_ligero_prover* const* pr, size_t nb, const void* h_u_ldt,
                             const void* const* d_dense, size_t ndense, const uint64_t* scale /*[nb][2]*/,
                             const uint64_t* const* h_idx, const void* const* h_val, const size_t* nsparse /*[nb]*/,
                             const void* h_u_quad, void* h_y_ldt, void* h_y_dot, void* h_y_q0, void* h_y_q2);
int lfgpu_ligero_open_batch(lfgpu_ctx* ctx, lfgpu_ligero_prover* const* pr, size_t nb, const size_t* idx /*[nb][nreq]*/,
                            void* h_req, uint8_t* h_nonces, uint8_t* h_path, size_t path_cap, size_t* npath /*[nb]*/);
/* ---- the same two over Fp256Base: nb provers from lfgpu_ligero_commit(field = LFGPU_FIELD_P256) of ONE context and ONE
 * lfgpu_ligero_param ----
 * Semantics, argument layout and error rules are those of lfgpu_ligero_prove_batch / lfgpu_ligero_open_batch with 32-byte
 * Montgomery images throughout (scale: [nb][4]; every element count above is in 32-byte elements).  Per chain of statements:
 * one upload, one memset, one dense and one sparse launch for the A rows of all statements (the sparse lists ragged, 0 terms
 * allowed), ONE lfgpu_fp256_rs_encode_rows over the chain's nwqrow rows per statement (they stand contiguously), the dot-proof,
 * low-degree and quadratic combinations (one launch each) and one read-back of all three y vectors; the opening is one column
 * gather, one digest gather and one read-back.  Results are byte-identical per statement to lfgpu_ligero_low_degree_proof,
 * lfgpu_ligero_dot_proof (A = scale * dense + the sparse terms, as the ZK path builds it), lfgpu_ligero_quadratic_proof and
 * lfgpu_ligero_open on that prover alone.  The reference's sanity check is made per statement: LFGPU_ERR_ASSERT naming the
 * statement whose y_quad has a non-zero W part.  Statements are chunked so that a chain's working set and the encoder's
 * scratch stay under 256 MiB; LFGPU_LP_CHUNK overrides (read once).
 * LFGPU_ERR_ARG, found before anything is enqueued: a NULL entry, nb out of 1..LFGPU_SC_BATCH_MAX, a prover of a 16-byte field
 * or of another context, provers whose lfgpu_ligero_param differ, the same prover twice, a prover without a commitment, a
 * sparse index out of range or not strictly increasing, an opened index out of range or given twice, a path buffer too small,
 * a dense block inside the call's scratch.  LFGPU_ERR_UNSUPPORTED: a sharded prover or one that holds a slab.
 * The commit of nb such provers in one chain is lfgpu_ligero_commit_batch256 above (lfgpu_column_commit_batch /
 * lfgpu_ligero_commit_batch keep refusing the field). */
int lfgpu_ligero_prove_batch256(lfgpu_ctx* ctx, lfgpu_ligero_prover* const* pr, size_t nb, const void* h_u_ldt,
                                const void* const* d_dense, size_t ndense, const uint64_t* scale /*[nb][4]*/,
                                const uint64_t* const* h_idx, const void* const* h_val, const size_t* nsparse /*[nb]*/,
                                const void* h_u_quad, void* h_y_ldt, void* h_y_dot, void* h_y_q0, void* h_y_q2);
int lfgpu_ligero_open_batch256(lfgpu_ctx* ctx, lfgpu_ligero_prover* const* pr, size_t nb, const size_t* idx /*[nb][nreq]*/,
                               void* h_req, uint8_t* h_nonces, uint8_t* h_path, size_t path_cap, size_t* npath /*[nb]*/);
/* device pointer of the resident tableau (nrow x block_enc elements of the prover's field: 16 bytes, P256 32) */
int lfgpu_ligero_tableau(lfgpu_ligero_prover* pr, void** d_T);
int lfgpu_ligero_free(lfgpu_ligero_prover* pr);

/* ---- host-buffer conveniences (what the header-only adapters call) ---------- */
int lfgpu_fp128_fft_host(lfgpu_ctx* ctx, int dir, size_t n, const uint64_t omega[2], uint64_t omega_order,
                         void* h_A);
int lfgpu_f64_2_fft_host(lfgpu_ctx* ctx, int dir, size_t n, const uint64_t omega[2], uint64_t omega_order,
                         void* h_A);
int lfgpu_gf2128_lch14_fft_host(lfgpu_ctx* ctx, int subfield_log_bits, int dir, unsigned l, uint64_t coset,
                                void* h_B);
int lfgpu_gf2128_rs_encode_rows_host(lfgpu_ctx* ctx, int subfield_log_bits, size_t nrow, size_t n, size_t m,
                                     void* h_T, size_t ld);
int lfgpu_fp128_rs_encode_rows_host(lfgpu_ctx* ctx, size_t nrow, size_t n, size_t m, const uint64_t omega[2],
                                    uint64_t omega_order, void* h_T, size_t ld);
int lfgpu_column_commit_host(lfgpu_ctx* ctx, int field, size_t nrow, size_t ld, size_t col0, size_t ncols,
                             const void* h_T, const uint8_t* h_nonces, uint8_t* h_layers,
                             uint8_t root_out[32]);

#ifdef __cplusplus
}
#endif
#endif /* LFGPU_H_ */
