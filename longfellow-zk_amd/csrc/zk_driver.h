// zk_driver.h -- the host driver around the protocol layer of zk_proto.h, written once over the same per-width policy P: the
// prover and batch records with their allocations, the handle checks of the batch entry points, ZkProver::commit for one prover
// and for a batch, the glue in front of zkp::prove / zkp::prove_batch, and LigeroProver::prove / LigeroVerifier::verify on a
// caller's term list.  zk.hip (P16) and zk256.hip (P32) instantiate it; the C entry points stay theirs.
//
// On top of what zk_proto.h asks of a policy, this layer wants:
//   kName, kCommitName, kCommitBatchName, kBatchNewName   the prefixes of the messages
//   kLigeroK                       the subfield_log_bits of lfgpu_ligero_param_init (4; 0 for Fp256Base)
//   ProverExtra                    what a prover keeps per width, with init(c, field, k, ninputs, mem) and a member d_eq: P16 the
//                                  SubfieldSolver of the wire format, P32 its own EQ table over the inputs
//   make(c, field, k, extra)       the policy object of a prover (extra == nullptr: a verifier)
//   ts_ok(c, ops)                  P32: the transcript must have the sized hooks
//   lig_commit, lig_commit_batch, lig_free, draws_only    the Ligero commit behind the C ABI or below it
//   eq_store(c, ninputs, own, &d_eq)   where the EQ table over the inputs goes: P16 the context's table, P32 `own`
//   batch_prepare(c, ninputs)      what a new batch readies on the context
//   ligero_param_ok(p)             the extra parameter checks of the term-list entry points
#pragma once
#include <memory>

#include "zk_proto.h"

namespace zkp {
namespace {
// The device and pinned allocations of a record, each with its byte size, recorded when it is made.  The scrub at destruction
// reads nothing else -- in particular not the circuit handle, which the caller may have freed first.
struct Owned {
  struct Dev {
    void* p;
    size_t bytes;
    bool secret;  // a function of a witness: cleared before the memory goes back to the allocator
  };
  lfgpu_ctx* c = nullptr;
  std::vector<Dev> dev;
  void* pinned = nullptr;
  size_t pinned_bytes = 0;
  bool alloc(void** p, size_t bytes, bool secret) {
    if (hipMalloc(p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      *p = nullptr;
      return false;
    }
    dev.push_back({*p, bytes, secret});
    return true;
  }
  bool alloc_pinned(void** p, size_t bytes) {
    if (hipHostMalloc(p, bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      *p = nullptr;
      return false;
    }
    pinned = *p;
    pinned_bytes = bytes;
    return true;
  }
  ~Owned() {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (const Dev& d : dev)
      if (d.secret) (void)hipMemsetAsync(d.p, 0, d.bytes, c->stream);
    (void)hipStreamSynchronize(c->stream);
    for (const Dev& d : dev) (void)hipFree(d.p);
    if (pinned) {
      memset(pinned, 0, pinned_bytes);
      (void)hipHostFree(pinned);
    }
  }
};

// ------------------------------------------------------------------ ZkProver
template <class P>
struct Prover {
  lfgpu_ctx* c = nullptr;
  const lfgpu_circuit* C = nullptr;  // for the calls on a live prover; the destructor does not look at it
  ProverState<P> st;                 // pads, the held proof, its wire bytes, timings
  typename P::ProverExtra ex;
  typename P::Lig* lp = nullptr;
  // device buffers of the layer inputs (eval_circuit), resident for the sumcheck, and the circuit output: functions of the
  // witness, scrubbed (as the Ligero tableau is by lig_free; the host copies of the pads: ~ProverState)
  std::vector<void*> d_in;
  void* d_V = nullptr;
  void* h_V = nullptr;  // pinned: outputs (nv elements) then the assert-zero flag, read back without blocking the host
  // lfgpu_zk_prover_set_comm: Ligero tableaux of at least comm_min_bytes are committed with their rows sharded over the
  // communicator's GPUs; everything else -- and the whole sumcheck -- runs replicated
  bool have_comm = false;
  lfgpu_comm_ops comm{};
  size_t comm_min_bytes = 0;
  Owned mem;
  P policy() const { return P::make(c, C->info.field, P::kLigeroK, &ex); }
  void drop_commitment() {  // ... and the proof made on it
    if (lp) P::lig_free(lp);
    lp = nullptr;
    st.have_proof = false;
    st.wire_valid = false;
  }
  ~Prover() {
    if (lp) P::lig_free(lp);
  }
};

template <class P>
int prover_init(Prover<P>& z, lfgpu_ctx* c, const lfgpu_circuit* C, size_t rateinv, size_t nreq, size_t block_enc) {
  z.c = c;
  z.C = C;
  z.st.init(C);
  // ZkProof: LigeroParam(n_witness + pad_size, nl quadratic constraints, rate, nreq[, block_enc]) (zk_proof.h:63-76)
  LF_TRY(lfgpu_ligero_param_init(&z.st.param, C->info.field, P::kLigeroK, z.st.n_witness + z.st.pad_size, C->info.nl, rateinv, nreq, block_enc));
  LF_HIP(c, hipSetDevice(c->device));
  z.mem.c = c;
  z.d_in.assign(C->layers.size(), nullptr);
  for (size_t l = 0; l < C->layers.size(); ++l)
    if (!z.mem.alloc(&z.d_in[l], C->layers[l].nw * P::kBytes, true)) return lf_fail(c, LFGPU_ERR_NOMEM, "%s: layer %zu inputs", P::kName, l);
  if (!z.mem.alloc(&z.d_V, C->info.nv * P::kBytes, true)) return lf_fail(c, LFGPU_ERR_NOMEM, "%s: outputs", P::kName);
  LF_TRY(z.ex.init(c, C->info.field, P::kLigeroK, C->info.ninputs, &z.mem));
  if (!z.mem.alloc_pinned(&z.h_V, C->info.nv * P::kBytes + 16)) return lf_fail(c, LFGPU_ERR_NOMEM, "%s: pinned outputs", P::kName);
  return LFGPU_OK;
}

template <class P>
void commit_done(Prover<P>& z, const lfgpu_transcript_ops* ts, uint8_t root_out[32], double t0) {
  ts->write_bytes(ts->user, z.st.proof.root, 32);  // LigeroTranscript::write_commitment
  if (root_out) memcpy(root_out, z.st.proof.root, 32);
  z.st.ms[0] = now_ms() - t0;
}

// ZkProver::commit (zk_prover.h:72-96) on one GPU, or with the tableau's rows sharded over the prover's communicator when it is
// above the threshold: witness || pads from rng, the Ligero commit, root -> transcript.
// draws_only: perform every RandomEngine draw of the commit (pads, then the Ligero layout) and stop -- rank 0 of a communicator
// records its engine's stream this way before any collective runs.
template <class P>
int commit(Prover<P>& z, const void* h_W, lfgpu_rng_fn rng, void* rng_user, const lfgpu_transcript_ops* ts, uint8_t root_out[32], bool draws_only = false) {
  lfgpu_ctx* c = z.c;
  LF_TRY(P::ts_ok(c, ts));
  const double t0 = now_ms();
  auto& st = z.st;
  LF_HIP(c, hipSetDevice(c->device));
  const P pol = z.policy();
  const typename P::Field F = pol.host_field(c);
  std::vector<typename P::E> Wv(st.param.nw);  // witness || pads
  LF_SCRUB_ON_EXIT(Wv);
  if (stage_witness(pol, F, z.C, st, h_W, c->rng_exact != 0, [&](uint8_t* b, size_t n) { rng(rng_user, b, n); }, Wv.data()) != st.param.nw)
    return lf_fail(c, LFGPU_ERR_ASSERT, "%s: witness layout", P::kCommitName);
  if (draws_only) return P::draws_only(c, st.param, Wv.data(), st.lqc.data(), rng, rng_user);
  z.drop_commitment();
  const bool shard_rows = z.have_comm && z.comm.world > 1 && st.param.nrow * st.param.block_enc * P::kBytes >= z.comm_min_bytes;
  LF_TRY(P::lig_commit(c, z.C->info, st.param, Wv.data(), st.lqc.data(), rng, rng_user, st.proof.root, &z.lp, shard_rows ? &z.comm : nullptr));
  commit_done(z, ts, root_out, t0);
  return LFGPU_OK;
}

// ZkProver::prove (zk_prover.h:98-149) on a committed prover
template <class P>
int prove(Prover<P>& z, const void* h_W, const lfgpu_transcript_ops* tso, int* ok) {
  LF_TRY(P::ts_ok(z.c, tso));
  if (!z.lp) return lf_fail(z.c, LFGPU_ERR_ARG, "%s: must run commit before prove", P::kProveName);
  auto eq_table = [&](typename P::E** d_eq) { return P::eq_store(z.c, z.C->info.ninputs, z.ex.d_eq, d_eq); };
  return prove<P>(z.c, z.C, z.policy(), z.st, z.lp, z.d_in.data(), z.d_V, z.h_V, eq_table, h_W, tso, ok);
}

// ------------------------------------------------------------------ a batch of provers of one circuit
// The batch owns what the lock-step needs nb_max times: the layers' input slabs (statement b of layer l at d_in[l] + b * ldw[l]
// elements), the outputs, one assert-zero flag per statement, their pinned read-back and nb_max EQ tables over the inputs (the
// dense blocks of the batched dot proofs).  All of it is allocated in batch_init and nothing is freed inside prove_batch (hipFree
// waits for every stream of the device); the only device memory a call may allocate is the context's pooled scratch, which
// grows on the first call at a shape.
template <class P>
struct Batch {
  lfgpu_ctx* c = nullptr;
  const lfgpu_circuit* C = nullptr;  // compared with the provers' and used by the calls; the destructor does not look at it
  size_t nb_max = 0;
  std::vector<void*> d_in;  // the slabs hold the wire values of every statement -- functions of the witnesses: scrubbed
  std::vector<size_t> ldw;
  void* d_V = nullptr;
  size_t ldv = 0;
  int* d_fail = nullptr;
  void* h_V = nullptr;
  void* d_eq = nullptr;  // [nb_max][ninputs]: functions of the challenges only, not scrubbed
  Owned mem;
  BatchBufs bufs() const { return BatchBufs{d_in.data(), ldw.data(), d_V, ldv, d_fail, h_V, nb_max, d_eq}; }
};

template <class P>
int batch_init(Batch<P>& bt, lfgpu_ctx* c, const lfgpu_circuit* C, size_t nb_max) {
  constexpr size_t B = P::kBytes, line = 64 / B;
  const char* who = P::kBatchNewName;
  bt.c = c;
  bt.C = C;
  bt.nb_max = nb_max;
  LF_HIP(c, hipSetDevice(c->device));
  bt.mem.c = c;
  auto pad = [](size_t n) { return (n + line - 1) / line * line; };  // slabs start on 64-byte lines
  const size_t nl = C->layers.size();
  bt.d_in.assign(nl, nullptr);
  bt.ldw.assign(nl, 0);
  for (size_t l = 0; l < nl; ++l) {
    bt.ldw[l] = pad(C->layers[l].nw);
    const size_t bytes = nb_max * bt.ldw[l] * B;
    if (!bt.mem.alloc(&bt.d_in[l], bytes, true)) return lf_fail(c, LFGPU_ERR_NOMEM, "%s: %zu slabs of layer %zu (%zu bytes)", who, nb_max, l, bytes);
  }
  bt.ldv = pad(C->info.nv);
  const size_t v_bytes = nb_max * bt.ldv * B;
  if (!bt.mem.alloc(&bt.d_V, v_bytes, true) || !bt.mem.alloc((void**)&bt.d_fail, nb_max * sizeof(int), false)) return lf_fail(c, LFGPU_ERR_NOMEM, "%s: outputs", who);
  if (!bt.mem.alloc_pinned(&bt.h_V, v_bytes + nb_max * sizeof(int))) return lf_fail(c, LFGPU_ERR_NOMEM, "%s: pinned outputs", who);
  if (!bt.mem.alloc(&bt.d_eq, std::max<size_t>(nb_max * C->info.ninputs, 1) * B, false))
    return lf_fail(c, LFGPU_ERR_NOMEM, "%s: %zu EQ tables over the inputs", who, nb_max);
  return P::batch_prepare(c, C->info.ninputs);  // here, not inside the first proof
}

// The handle checks of the four batch entry points (`who`), on the ABI's prover handles: nb, NULLs (rng == nullptr: the call
// takes no engines), one context, circuit and width, no communicator, no prover twice.  What is left -- a prover that has not
// committed, a transcript without the sized hooks, another LigeroParam -- is found by prove_batch / commit_batch below, after
// these and still before the first RandomEngine draw, transcript write or enqueue.
template <class Handle>
int check_batch_call(const char* who, lfgpu_ctx* c, const lfgpu_circuit* C, size_t nb_max, bool wide, Handle* const* zk, size_t nb, const void* const* h_W,
                     const lfgpu_rng_fn* rng, const lfgpu_transcript_ops* const* ts) {
  if (nb == 0 || nb > nb_max) return lf_fail(c, LFGPU_ERR_ARG, "%s: nb = %zu, the batch holds 1..%zu statements", who, nb, nb_max);
  for (size_t b = 0; b < nb; ++b) {
    if (!zk[b] || !h_W[b] || (rng && !rng[b]) || !ts[b]) return lf_fail(c, LFGPU_ERR_ARG, "%s: null argument for statement %zu", who, b);
    if (zk[b]->c != c || zk[b]->C != C || zk[b]->wide() != wide) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu belongs to another context or circuit", who, b);
    if (zk[b]->have_comm()) return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "%s: prover %zu has a communicator (the batch runs on one GPU)", who, b);
    for (size_t a = 0; a < b; ++a)
      if (zk[a] == zk[b]) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu appears twice", who, b);
  }
  return LFGPU_OK;
}

// ZkProver::prove for nb committed provers (Z: Prover<P> or a record derived from it) in lock-step: the glue in front of
// zkp::prove_batch of zk_proto.h
template <class P, class Z>
int prove_batch(Batch<P>& bt, Z* const* z, size_t nb, const void* const* h_W, const lfgpu_transcript_ops* const* ts, int* ok) {
  lfgpu_ctx* c = bt.c;
  for (size_t b = 0; b < nb; ++b) {
    LF_TRY(P::ts_ok(c, ts[b]));
    if (!z[b]->lp) return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu must run commit before prove", P::kProveBatchName, b);
  }
  std::vector<P> pol;
  std::vector<ProverState<P>*> st(nb);
  std::vector<typename P::Lig*> lp(nb);
  pol.reserve(nb);
  for (size_t b = 0; b < nb; ++b) {
    pol.push_back(z[b]->policy());
    st[b] = &z[b]->st;
    lp[b] = z[b]->lp;
  }
  // (the per-statement tail: one statement after the other in stream order)
  auto eq_table = [&](typename P::E** d_eq) { return P::eq_store(c, bt.C->info.ninputs, bt.d_eq, d_eq); };
  return prove_batch<P>(c, bt.C, pol.data(), st.data(), lp.data(), bt.bufs(), nb, eq_table, h_W, ts, ok);
}

// ZkProver::commit for nb provers: commit's one-GPU branch per statement around ONE batched Ligero commit
template <class P, class Z>
int commit_batch(Batch<P>& bt, Z* const* z, size_t nb, const void* const* h_W, const lfgpu_rng_fn* rng, void* const* rng_user,
                 const lfgpu_transcript_ops* const* ts, uint8_t* roots_out) {
  using E = typename P::E;
  lfgpu_ctx* c = bt.c;
  for (size_t b = 0; b < nb; ++b) {
    LF_TRY(P::ts_ok(c, ts[b]));
    if (memcmp(&z[b]->st.param, &z[0]->st.param, sizeof(lfgpu_ligero_param)) != 0)
      return lf_fail(c, LFGPU_ERR_ARG, "%s: prover %zu has another LigeroParam (rate, nreq or block_enc) than prover 0", P::kCommitBatchName, b);
  }
  const double t0 = now_ms();
  LF_HIP(c, hipSetDevice(c->device));
  const lfgpu_ligero_param& p = z[0]->st.param;
  // whatever happens from here on, no prover of the call keeps an earlier commitment or proof
  for (size_t b = 0; b < nb; ++b) z[b]->drop_commitment();
  // witness || pads of every statement; fill_pad's draws of statement b come from rng[b], before its Ligero draws (the pads of
  // ALL statements are drawn before the first Ligero layout: a statement's own order -- pads, then layout -- is the single
  // path's as long as its engine is its own, which the header asks for)
  std::vector<E> Wv(nb * p.nw);
  LF_SCRUB_ON_EXIT(Wv);
  std::vector<const E*> Wp(nb);
  std::vector<void*> users(nb);
  const typename P::Field F = z[0]->policy().host_field(c);
  for (size_t b = 0; b < nb; ++b) {
    lfgpu_rng_fn r = rng[b];
    void* u = users[b] = rng_user ? rng_user[b] : nullptr;
    E* W = Wv.data() + b * p.nw;
    if (stage_witness(z[b]->policy(), F, bt.C, z[b]->st, h_W[b], c->rng_exact != 0, [&](uint8_t* buf, size_t n) { r(u, buf, n); }, W) != p.nw)
      return lf_fail(c, LFGPU_ERR_ASSERT, "%s: witness layout (statement %zu)", P::kCommitBatchName, b);
    Wp[b] = W;
  }
  std::vector<uint8_t> roots(nb * 32);
  std::vector<typename P::Lig*> lps(nb, nullptr);
  // (the lqc triples are the circuit's: the same for every prover)
  LF_TRY(P::lig_commit_batch(c, bt.C->info, p, nb, Wp.data(), z[0]->st.lqc.data(), rng, users.data(), roots.data(), lps.data()));
  for (size_t b = 0; b < nb; ++b) {
    z[b]->lp = lps[b];
    memcpy(z[b]->st.proof.root, &roots[32 * b], 32);
    ts[b]->write_bytes(ts[b]->user, z[b]->st.proof.root, 32);  // LigeroTranscript::write_commitment
  }
  if (roots_out) memcpy(roots_out, roots.data(), nb * 32);
  const double dt = now_ms() - t0;
  for (size_t b = 0; b < nb; ++b) z[b]->st.ms[0] = dt;
  return LFGPU_OK;
}

// ------------------------------------------------------------------ LigeroProver::prove / LigeroVerifier::verify on a caller's statement
// A second, small driver over ligero_prove / ligero_verify / com_proof_write / com_proof_read: the ZK paths keep their own A step
// (dense EQ block + host-folded sparse terms), these two accumulate A on the device from the caller's term list (Term:
// lfgpu_ligero_llterm or lfgpu_ligero_llterm256).  The callers pass what differs per width: the checks in front (pre), and the
// dot step or the verifier's extension step over the term list.
// The host scan in front of the first transcript call or launch.
template <class P, class Term>
bool ligero_statement_ok(const lfgpu_ligero_param& p, size_t nl, size_t nllterm, const Term* llterm, const size_t* h_lqc) {
  if ((nllterm && !llterm) || (p.nq && !h_lqc)) return false;
  if (nllterm >= ((size_t)1 << 32) || nllterm + 6 * p.nq >= ((size_t)1 << 32)) return false;
  if (!P::ligero_param_ok(p)) return false;
  for (size_t t = 0; t < nllterm; ++t)
    if (llterm[t].c >= nl || llterm[t].w >= p.nw) return false;
  for (size_t i = 0; i < 3 * p.nq; ++i)
    if (h_lqc[i] >= p.nw) return false;
  return true;
}
#define LF_BAD_STATEMENT "%s: bad statement (null list, term with c >= nl or w >= nw, lqc index >= nw, or 2^32 summands)"
// the held serialisation into the caller's buffer; it stays held when the buffer is too small
inline int wire_copy_out(const char* who, const LfLigeroView& v, uint8_t* buf, size_t cap, size_t* nbytes) {
  *nbytes = v.wire->size();
  if (cap < v.wire->size()) return lf_fail(v.c, LFGPU_ERR_ARG, "%s: buffer too small (%zu < %zu)", who, cap, v.wire->size());
  memcpy(buf, v.wire->data(), v.wire->size());
  *v.wire_held = false;
  return LFGPU_OK;
}

// pre(view, &lig): the width's checks and its Ligero record; dot(lig, alphal, alphaq, y_dot): the dot proof with A from the terms
template <class P, class Term, class Pre, class Dot>
int ligero_prove_entry(const char* who, lfgpu_ligero_prover* lp, const lfgpu_transcript_ops* tso, size_t nl, size_t nllterm, const Term* llterm,
                       const uint8_t hash_of_llterm[32], const size_t* h_lqc, uint8_t* buf, size_t cap, size_t* nbytes, Pre pre, Dot dot) {
  using E = typename P::E;
  if (!lp || !tso || !hash_of_llterm || !nbytes) return LFGPU_ERR_ARG;
  LfLigeroView v;
  lf_ligero_prover_view(lp, &v);
  lfgpu_ctx* c = v.c;
  const lfgpu_ligero_param& p = v.p;
  typename P::Lig* lig = nullptr;
  LF_TRY(pre(v, &lig));
  if (!ligero_statement_ok<P>(p, nl, nllterm, llterm, h_lqc)) return lf_fail(c, LFGPU_ERR_ARG, LF_BAD_STATEMENT, who);
  if (buf && *v.wire_held) return wire_copy_out(who, v, buf, cap, nbytes);  // the copy that follows a size query: the same serialisation
  *v.wire_held = false;
  LF_HIP(c, hipSetDevice(c->device));
  typename P::ProverExtra ex;
  LF_TRY(ex.init(c, v.field, v.k, 0, nullptr));
  const P pol = P::make(c, v.field, v.k, &ex);
  const Ts<P> ts{&pol, tso, tso->user};
  ComProof<E> pr;
  double tq[6];
  auto dot_fn = [&](const std::vector<E>& alphal, const std::vector<E>& alphaq, E* y_dot) { return dot(lig, alphal, alphaq, y_dot); };
  LF_TRY(ligero_prove<P>(p, lig, ts, hash_of_llterm, nl, dot_fn, pr, tq));
  static const bool verbose = getenv("LFGPU_VERBOSE") != nullptr;
  if (verbose)
    fprintf(stderr, "lfgpu %s: ldt %.2f ms | challenges %.2f | A from %zu terms + dot %.2f | quad %.2f | challenges+open %.2f\n", who, tq[1] - tq[0],
            tq[2] - tq[1], nllterm, tq[3] - tq[2], tq[4] - tq[3], tq[5] - tq[4]);
  v.wire->clear();
  com_proof_write(pol, pr, *v.wire);
  *v.wire_held = true;  // kept after a size query, and if the buffer turns out too small
  if (!buf) {
    *nbytes = v.wire->size();
    return LFGPU_OK;
  }
  return wire_copy_out(who, v, buf, cap, nbytes);
}

// pre(): the width's checks; ext(pr, alphal, alphaq, idx, out): ligero_verify's device step with the A rows from the terms
template <class P, class Term, class Pre, class Ext>
int ligero_verify_entry(const char* who, lfgpu_ctx* c, int field, int k, const lfgpu_ligero_param* pp, const uint8_t root[32], const uint8_t* proof,
                        size_t proof_len, const lfgpu_transcript_ops* tso, size_t nl, size_t nllterm, const Term* llterm, const uint8_t hash_of_llterm[32],
                        const void* h_b, const size_t* h_lqc, int* ok, const char** why_out, Pre pre, Ext ext) {
  using E = typename P::E;
  if (!c || !pp || !root || !proof || !tso || !hash_of_llterm || !ok || (nl && !h_b)) return lf_fail(c, LFGPU_ERR_ARG, "%s: null argument", who);
  *ok = 0;
  LF_TRY(pre());
  const lfgpu_ligero_param& p = *pp;
  if (!ligero_statement_ok<P>(p, nl, nllterm, llterm, h_lqc)) return lf_fail(c, LFGPU_ERR_ARG, LF_BAD_STATEMENT, who);
  const P pol = P::make(c, field, k, nullptr);
  const typename P::Field F = pol.host_field(c);
  auto fail = [&](int w) {
    if (why_out) *why_out = why_string(w);
    return (int)LFGPU_OK;
  };
  ComProof<E> pr;
  WireReader<P> rd{pol, proof, proof_len};
  if (!com_proof_read(rd, p, pr) || rd.bad || rd.left != 0) return fail(kWhyParse);
  LF_HIP(c, hipSetDevice(c->device));
  const Ts<P> ts{&pol, tso, tso->user};
  auto ext_fn = [&](const std::vector<E>& alphal, const std::vector<E>& alphaq, const size_t* idx, std::vector<E>& out) {
    return ext(pr, alphal, alphaq, idx, out);
  };
  int w = kWhyOk;
  double tv[6];
  LF_TRY(ligero_verify<P>(pol, F, p, root, pr, ts, hash_of_llterm, nl, (const E*)h_b, ext_fn, &w, tv));
  if (w == kWhyOk) *ok = 1;
  return fail(w);
}
}  // namespace
}  // namespace zkp
