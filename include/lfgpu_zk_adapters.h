// lfgpu_zk_adapters.h -- header-only C++17 adapter that presents the reference's ZkProver on top of the prover-level C ABI
// (include/lfgpu_zk.h).  Where lfgpu_adapters.h swaps a template argument INSIDE the reference's prover (the Reed-Solomon
// interpolator), this one swaps the prover itself: the caller keeps its Circuit, Dense, ZkProof, Transcript and
// RandomEngine objects and its two calls,
//
//     ZkProver<Field, RSFactory> p(circuit, F, rsf);      ->   lfgpu::GpuZkProver<Field, proofs::ReadBuffer> p(ctx, lfc1, len, F);
//     p.commit(zkp, W, tp, rng);                                p.commit(zkp, W, tp, rng);
//     if (!p.prove(zkp, W, tp)) ...                             if (!p.prove(zkp, W, tp)) ...
//
// (reference lib/zk/zk_prover.h:60-149; call sites lib/circuits/mdoc/mdoc_zk.cc:494-522, the body of run_mdoc_prover.)
// Evaluation of the circuit, the padded sumcheck, the constraint replay and the Ligero commit / prove then run in
// liblfgpu.so (csrc/zk.hip for GF2_128 / Fp128, csrc/zk256.hip for Fp256Base); the Fiat-Shamir transcript and the random
// engine stay the CALLER's objects, reached through hooks, so the bytes written to / drawn from them are the reference's.
// The proof comes back through ZkProof::read on the wire bytes, i.e. in exactly the form a verifier would receive it.
//
// lfgpu::GpuZkVerifier<Field> does the same for ZkVerifier (recv_commitment / verify).
//
// `lfc1` = the circuit in the reference's own serialisation (CircuitWriter::to_bytes, or the span of the decompressed
// circuit file that CircuitReader::from_bytes consumed for this circuit).  This header includes no reference header.
#ifndef LFGPU_ZK_ADAPTERS_H_
#define LFGPU_ZK_ADAPTERS_H_

#include <cstddef>
#include <optional>

#include "lfgpu_adapters.h"
#include "lfgpu_zk.h"

namespace lfgpu {

namespace detail {
// the caller's Transcript (lib/random/transcript.h:70-190) behind lfgpu_transcript_ops
template <class Field, class TranscriptT>
struct TranscriptHook {
  using Elt = typename Field::Elt;
  TranscriptT* t;
  const Field* F;
  std::unique_ptr<TranscriptT> owned;  // clones own their transcript
  static TranscriptHook* self(void* u) { return static_cast<TranscriptHook*>(u); }
  static Elt elt(const Field& F, const uint8_t* image) {
    auto e = F.of_bytes_field(image);  // the library only ever hands over images of field elements
    if (!e.has_value()) check(nullptr, LFGPU_ERR_ASSERT, "transcript hook: not a field element");
    return e.value();
  }
  static void write_bytes(void* u, const uint8_t* d, size_t n) { self(u)->t->write(d, n); }
  static void write_elt(void* u, const uint8_t* e) { self(u)->t->write(elt(*self(u)->F, e), *self(u)->F); }
  static void write_elt_array(void* u, const uint8_t* e, size_t n) {
    std::vector<Elt> v(n ? n : 1);
    for (size_t i = 0; i < n; ++i) v[i] = elt(*self(u)->F, e + Field::kBytes * i);
    self(u)->t->write(v.data(), 1, n, *self(u)->F);
  }
  static void write_elt_sized(void* u, const uint8_t* e, size_t) { write_elt(u, e); }
  static void write_elt_array_sized(void* u, const uint8_t* e, size_t n, size_t) { write_elt_array(u, e, n); }
  static void gen_bytes(void* u, uint8_t* o, size_t n) { self(u)->t->bytes(o, n); }
  static void* clone(void* u) {  // Transcript::clone (:95-99); guaranteed elision: Transcript has no copy / move constructor
    TranscriptHook* h = new TranscriptHook{nullptr, self(u)->F, nullptr};
    h->owned.reset(new TranscriptT(self(u)->t->clone()));
    h->t = h->owned.get();
    return h;
  }
  static void free_clone(void* u) { delete self(u); }
  lfgpu_transcript_ops ops() {
    lfgpu_transcript_ops o;
    o.user = this;
    o.write_bytes = write_bytes;
    o.write_elt = write_elt;
    o.write_elt_array = write_elt_array;
    o.gen_bytes = gen_bytes;
    o.clone = clone;
    o.free_clone = free_clone;
    o.write_elt_sized = write_elt_sized;
    o.write_elt_array_sized = write_elt_array_sized;
    return o;
  }
};
template <class RandomEngineT>
void rng_hook(void* user, uint8_t* buf, size_t n) {  // RandomEngine::bytes (lib/random/random.h:32-35)
  static_cast<RandomEngineT*>(user)->bytes(buf, n);
}
}  // namespace detail

// Drop-in for ZkProver<Field, ReedSolomonFactory> (lib/zk/zk_prover.h:45-149).  ReadBufferT = proofs::ReadBuffer.
template <class Field, class ReadBufferT>
class GpuZkProver {
 public:
  // comm != nullptr: one process per GPU, every rank constructs the prover on its own Context and calls commit / prove with the
  // same arguments (SPMD; only rank 0's RandomEngine is drawn from).  Ligero tableaux of at least min_tableau_bytes are
  // committed with their rows sharded over the communicator's GPUs (lfgpu_zk_prover_set_comm, include/lfgpu_zk.h); the hooks
  // are the caller's binding of all_gather / all_to_all / broadcast to RCCL.  All three fields.
  GpuZkProver(const Context& ctx, const uint8_t* lfc1, size_t len, const Field& F, const lfgpu_comm_ops* comm = nullptr, size_t min_tableau_bytes = 0)
      : c_(ctx), f_(F), have_comm_(comm != nullptr), min_tableau_bytes_(min_tableau_bytes) {
    if (comm) comm_ = *comm;
    check(c_.get(), lfgpu_circuit_from_lfc1(c_.get(), lfc1, len, &circuit_), "lfgpu_circuit_from_lfc1");
  }
  ~GpuZkProver() {
    if (zk_) lfgpu_zk_prover_free(zk_);
    if (circuit_) lfgpu_circuit_free(circuit_);
  }
  GpuZkProver(const GpuZkProver&) = delete;
  GpuZkProver& operator=(const GpuZkProver&) = delete;

  // ZkProver::commit (zk_prover.h:72-96).  zkp.param carries rate, nreq and block_enc as the ZkProof constructor set them.
  template <class ZkProofT, class DenseT, class TranscriptT, class RandomEngineT>
  void commit(ZkProofT& zkp, const DenseT& W, TranscriptT& tp, RandomEngineT& rng) {
    if (!zk_) {
      check(c_.get(), lfgpu_zk_prover_new(c_.get(), circuit_, zkp.param.rateinv, zkp.param.nreq, zkp.param.block_enc, &zk_), "lfgpu_zk_prover_new");
      if (have_comm_) check(c_.get(), lfgpu_zk_prover_set_comm(zk_, &comm_, min_tableau_bytes_), "lfgpu_zk_prover_set_comm");
      lfgpu_ligero_param p;
      check(c_.get(), lfgpu_zk_prover_param(zk_, &p), "lfgpu_zk_prover_param");
      if (p.nrow != zkp.param.nrow || p.block != zkp.param.block || p.nw != zkp.param.nw || p.block_ext != zkp.param.block_ext)
        check(c_.get(), LFGPU_ERR_ASSERT, "GpuZkProver: Ligero parameters differ from the caller's ZkProof");
    }
    detail::TranscriptHook<Field, TranscriptT> hook{&tp, &f_, nullptr};
    const lfgpu_transcript_ops ops = hook.ops();
    uint8_t root[32];
    check(c_.get(), lfgpu_zk_commit(zk_, W.v_.data(), detail::rng_hook<RandomEngineT>, &rng, &ops, root), "lfgpu_zk_commit");
    std::memcpy(zkp.com.root.data, root, 32);
  }

  // ZkProver::prove (zk_prover.h:98-149): false when the witness does not satisfy the circuit
  template <class ZkProofT, class DenseT, class TranscriptT>
  bool prove(ZkProofT& zkp, const DenseT& W, TranscriptT& tp) {
    if (!zk_) check(c_.get(), LFGPU_ERR_ARG, "must run commit before prove");
    detail::TranscriptHook<Field, TranscriptT> hook{&tp, &f_, nullptr};
    const lfgpu_transcript_ops ops = hook.ops();
    int ok = 0;
    check(c_.get(), lfgpu_zk_prove(zk_, W.v_.data(), &ops, &ok), "lfgpu_zk_prove");
    if (!ok) return false;
    size_t n = 0;
    check(c_.get(), lfgpu_zk_proof_write(zk_, nullptr, 0, &n), "lfgpu_zk_proof_write");
    std::vector<uint8_t> wire(n);
    check(c_.get(), lfgpu_zk_proof_write(zk_, wire.data(), wire.size(), &n), "lfgpu_zk_proof_write");
    ReadBufferT rb(wire.data(), n);
    if (!zkp.read(rb, f_)) check(c_.get(), LFGPU_ERR_ASSERT, "GpuZkProver: ZkProof::read rejected the library's wire bytes");
    return true;
  }
  // host milliseconds of the last commit / prove by phase (lfgpu_zk_timings)
  void timings(double ms[6]) const { check(c_.get(), lfgpu_zk_timings(zk_, ms), "lfgpu_zk_timings"); }

 private:
  const Context& c_;
  const Field& f_;
  lfgpu_circuit* circuit_ = nullptr;
  lfgpu_zk_prover* zk_ = nullptr;
  bool have_comm_ = false;
  lfgpu_comm_ops comm_{};
  size_t min_tableau_bytes_ = 0;
};

// Drop-in for ZkVerifier<Field, ReedSolomonFactory> (lib/zk/zk_verifier.h:42-94; call sites lib/circuits/mdoc/mdoc_zk.cc:669-705):
// recv_commitment writes the commitment to the caller's transcript exactly as LigeroTranscript::write_commitment does,
// verify serialises the caller's ZkProof with its own ZkProof::write and hands the wire bytes to lfgpu_zk_verify_committed.
template <class Field>
class GpuZkVerifier {
 public:
  GpuZkVerifier(const Context& ctx, const uint8_t* lfc1, size_t len, size_t rate, size_t nreq, size_t block_enc, const Field& F)
      : c_(ctx), f_(F), rate_(rate), nreq_(nreq), block_enc_(block_enc) {
    check(c_.get(), lfgpu_circuit_from_lfc1(c_.get(), lfc1, len, &circuit_), "lfgpu_circuit_from_lfc1");
  }
  ~GpuZkVerifier() {
    if (circuit_) lfgpu_circuit_free(circuit_);
  }
  GpuZkVerifier(const GpuZkVerifier&) = delete;
  GpuZkVerifier& operator=(const GpuZkVerifier&) = delete;

  template <class ZkProofT, class TranscriptT>
  void recv_commitment(const ZkProofT& zk, TranscriptT& t) const {
    t.write(zk.com.root.data, 32);
  }
  template <class ZkProofT, class DenseT, class TranscriptT>
  bool verify(const ZkProofT& zk, const DenseT& pub, TranscriptT& tv) const {
    std::vector<uint8_t> wire;
    zk.write(wire, f_);
    detail::TranscriptHook<Field, TranscriptT> hook{&tv, &f_, nullptr};
    const lfgpu_transcript_ops ops = hook.ops();
    int ok = 0;
    const char* why = nullptr;
    check(c_.get(),
          lfgpu_zk_verify_committed(c_.get(), circuit_, rate_, nreq_, block_enc_, wire.data(), wire.size(), pub.v_.data(), &ops, &ok, &why),
          "lfgpu_zk_verify_committed");
    if (!ok && why) std::fprintf(stderr, "lfgpu: verify failed: %s\n", why);
    return ok != 0;
  }

 private:
  const Context& c_;
  const Field& f_;
  size_t rate_, nreq_, block_enc_;
  lfgpu_circuit* circuit_ = nullptr;
};

// ---- LigeroProver / LigeroVerifier (lib/ligero/ligero_prover.h:34-146, ligero_verifier.h:30-123) on a caller's own statement:
//
//     LigeroProver<Field, RSFactory> lp(param);               ->   lfgpu::GpuLigeroProver<Field> lp(ctx, param);
//     lp.commit(com, ts, W, sfb, lqc, rsf, rng, F);                 lp.commit(com, ts, W, sfb, lqc, rng, F);
//     lp.prove(proof, ts, nl, nllterm, llterm, h, lqc, rsf, F);     lp.prove(proof, ts, nl, nllterm, llterm, h, lqc, F);
//     LigeroVerifier<Field, RSFactory>::verify(&why, param, com, proof, ts, nl, nllterm, llterm, h, b, lqc, rsf, F)
//                                                              ->   lfgpu::GpuLigeroVerifier<Field>(ctx).verify(&why, param, com, proof, ts, nl, ..., b, lqc, F)
//
// The argument types are the reference's (LigeroParam, LigeroCommitment, LigeroProof, LigeroLinearConstraint<Field>[],
// LigeroHash, LigeroQuadraticConstraint[], Transcript, RandomEngine); only the interpolator factory is gone.  The proof crosses
// the C ABI as the write_com_proof bytes (lib/zk/zk_proof.h:137-185), converted from / to the caller's LigeroProof below with the
// Field's own to_bytes / of_bytes functions.  GF2_128<k>, Fp128 and Fp256Base (the last through lfgpu_ligero_prove256 /
// lfgpu_ligero_verify256: its term record holds a 32-byte coefficient).
namespace detail {
constexpr size_t kComMaxRunLen = size_t{1} << 25;
template <class Field, class LigeroProofT>
void com_proof_to_wire(const LigeroProofT& pr, const Field& F, std::vector<uint8_t>& o) {
  uint8_t b[Field::kBytes];
  auto put = [&](const typename Field::Elt& e) {
    F.to_bytes_field(b, e);
    o.insert(o.end(), b, b + Field::kBytes);
  };
  auto put_size = [&](size_t n) {
    for (int i = 0; i < 4; ++i) o.push_back(static_cast<uint8_t>(n >> (8 * i)));
  };
  for (const auto& e : pr.y_ldt) put(e);
  for (const auto& e : pr.y_dot) put(e);
  for (const auto& e : pr.y_quad_0) put(e);
  for (const auto& e : pr.y_quad_2) put(e);
  for (const auto& n : pr.merkle.nonce) o.insert(o.end(), n.bytes, n.bytes + 32);
  bool sub = false;  // alternating full-field / subfield runs, the first one full-field (possibly empty)
  for (size_t i = 0, n = pr.req.size(); i < n; sub = !sub) {
    size_t len = 0;
    while (i + len < n && len < kComMaxRunLen && F.in_subfield(pr.req[i + len]) == sub) ++len;
    put_size(len);
    for (size_t j = i; j < i + len; ++j) {
      if (sub) {
        F.to_bytes_subfield(b, pr.req[j]);
        o.insert(o.end(), b, b + Field::kSubFieldBytes);
      } else {
        put(pr.req[j]);
      }
    }
    i += len;
  }
  put_size(pr.merkle.path.size());
  for (const auto& d : pr.merkle.path) o.insert(o.end(), d.data, d.data + 32);
}
template <class Field, class LigeroProofT>
bool com_proof_of_wire(LigeroProofT& pr, const Field& F, const uint8_t* q, size_t left) {
  auto take = [&](size_t n) {
    const uint8_t* r = q;
    q += n;
    left -= n;
    return r;
  };
  auto get = [&](typename Field::Elt& e) {
    if (left < Field::kBytes) return false;
    auto v = F.of_bytes_field(take(Field::kBytes));
    if (!v.has_value()) return false;
    e = v.value();
    return true;
  };
  auto get_size = [&](size_t& n) {
    if (left < 4) return false;
    const uint8_t* b = take(4);
    n = size_t{b[0]} | size_t{b[1]} << 8 | size_t{b[2]} << 16 | size_t{b[3]} << 24;
    return true;
  };
  for (auto& e : pr.y_ldt)
    if (!get(e)) return false;
  for (auto& e : pr.y_dot)
    if (!get(e)) return false;
  for (auto& e : pr.y_quad_0)
    if (!get(e)) return false;
  for (auto& e : pr.y_quad_2)
    if (!get(e)) return false;
  for (auto& n : pr.merkle.nonce) {
    if (left < 32) return false;
    std::memcpy(n.bytes, take(32), 32);
  }
  bool sub = false;
  for (size_t i = 0, n = pr.req.size(); i < n; sub = !sub) {
    size_t len = 0;
    if (!get_size(len) || len > n - i) return false;
    for (size_t j = i; j < i + len; ++j) {
      if (sub) {
        if (left < Field::kSubFieldBytes) return false;
        auto v = F.of_bytes_subfield(take(Field::kSubFieldBytes));
        if (!v.has_value()) return false;
        pr.req[j] = v.value();
      } else if (!get(pr.req[j])) {
        return false;
      }
    }
    i += len;
  }
  size_t npath = 0;
  if (!get_size(npath) || left != npath * 32) return false;
  pr.merkle.path.resize(npath);
  for (auto& d : pr.merkle.path) std::memcpy(d.data, take(32), 32);
  return true;
}
// the reference's constraint records are the C ABI's: { size_t c, w; Elt k } and { size_t x, y, z }
template <class LlT>
const lfgpu_ligero_llterm* llterm_image(const LlT* llterm) {
  static_assert(sizeof(LlT) == sizeof(lfgpu_ligero_llterm) && offsetof(LlT, k) == offsetof(lfgpu_ligero_llterm, k), "LigeroLinearConstraint image");
  return reinterpret_cast<const lfgpu_ligero_llterm*>(llterm);
}
template <class LlT>
const lfgpu_ligero_llterm256* llterm256_image(const LlT* llterm) {  // Fp256Base: k is the 32-byte Montgomery image
  static_assert(sizeof(LlT) == sizeof(lfgpu_ligero_llterm256) && offsetof(LlT, k) == offsetof(lfgpu_ligero_llterm256, k), "LigeroLinearConstraint image");
  return reinterpret_cast<const lfgpu_ligero_llterm256*>(llterm);
}
// lfgpu_ligero_prove, or lfgpu_ligero_prove256 for Fp256Base
template <class Field, class LlT>
int ligero_prove_call(lfgpu_ligero_prover* lp, const lfgpu_transcript_ops* ops, size_t nl, size_t nllterm, const LlT* llterm, const uint8_t* hash,
                      const size_t* lqc, uint8_t* buf, size_t cap, size_t* n) {
  if constexpr (field_id<Field>() == LFGPU_FIELD_P256) {
    return lfgpu_ligero_prove256(lp, ops, nl, nllterm, llterm256_image(llterm), hash, lqc, buf, cap, n);
  } else {
    return lfgpu_ligero_prove(lp, ops, nl, nllterm, llterm_image(llterm), hash, lqc, buf, cap, n);
  }
}
template <class LqcT>
const size_t* lqc_image(const LqcT* lqc) {
  static_assert(sizeof(LqcT) == 3 * sizeof(size_t), "LigeroQuadraticConstraint image");
  return reinterpret_cast<const size_t*>(lqc);
}
template <class Field, class ParamT>
lfgpu_ligero_param ligero_param_of(lfgpu_ctx* ctx, const ParamT& p) {
  lfgpu_ligero_param q;
  check(ctx, lfgpu_ligero_param_init(&q, field_id<Field>(), subfield_log_bits<Field>(), p.nw, p.nq, p.rateinv, p.nreq, p.block_enc), "lfgpu_ligero_param_init");
  if (q.nrow != p.nrow || q.block != p.block || q.dblock != p.dblock || q.block_ext != p.block_ext || q.w != p.w)
    check(ctx, LFGPU_ERR_ASSERT, "Ligero parameters differ from the caller's LigeroParam");
  return q;
}
}  // namespace detail

template <class Field>
class GpuLigeroProver {
  using Elt = typename Field::Elt;

 public:
  template <class ParamT>
  GpuLigeroProver(const Context& ctx, const ParamT& p) : c_(ctx), p_(detail::ligero_param_of<Field>(ctx.get(), p)) {}
  ~GpuLigeroProver() {
    if (lp_) lfgpu_ligero_free(lp_);
  }
  GpuLigeroProver(const GpuLigeroProver&) = delete;
  GpuLigeroProver& operator=(const GpuLigeroProver&) = delete;

  // LigeroProver::commit (ligero_prover.h:58-79), the root written to ts as LigeroTranscript::write_commitment does
  template <class CommitmentT, class TranscriptT, class LqcT, class RandomEngineT>
  void commit(CommitmentT& com, TranscriptT& ts, const Elt W[], size_t subfield_boundary, const LqcT lqc[], RandomEngineT& rng, const Field&) {
    if (lp_) lfgpu_ligero_free(lp_);
    lp_ = nullptr;
    uint8_t root[32];
    check(c_.get(),
          lfgpu_ligero_commit(c_.get(), field_id<Field>(), subfield_log_bits<Field>(), &p_, W, subfield_boundary, detail::lqc_image(lqc),
                              detail::rng_hook<RandomEngineT>, &rng, root, &lp_),
          "lfgpu_ligero_commit");
    std::memcpy(com.root.data, root, 32);
    ts.write(com.root.data, 32);
  }

  // LigeroProver::prove (ligero_prover.h:84-146)
  template <class ProofT, class TranscriptT, class LlT, class HashT, class LqcT>
  void prove(ProofT& proof, TranscriptT& ts, size_t nl, size_t nllterm, const LlT llterm[], const HashT& hash_of_llterm, const LqcT lqc[], const Field& F) {
    if (!lp_) check(c_.get(), LFGPU_ERR_ARG, "must run commit before prove");
    detail::TranscriptHook<Field, TranscriptT> hook{&ts, &F, nullptr};
    const lfgpu_transcript_ops ops = hook.ops();
    size_t n = 0;  // the size query runs the proof; the second call copies the held bytes
    check(c_.get(), detail::ligero_prove_call<Field>(lp_, &ops, nl, nllterm, llterm, hash_of_llterm.bytes, detail::lqc_image(lqc), nullptr, 0, &n),
          "lfgpu_ligero_prove");
    std::vector<uint8_t> wire(n);
    check(c_.get(), detail::ligero_prove_call<Field>(lp_, &ops, nl, nllterm, llterm, hash_of_llterm.bytes, detail::lqc_image(lqc), wire.data(), n, &n),
          "lfgpu_ligero_prove");
    if (!detail::com_proof_of_wire(proof, F, wire.data(), n)) check(c_.get(), LFGPU_ERR_ASSERT, "GpuLigeroProver: the library's wire bytes do not parse");
  }

 private:
  const Context& c_;
  lfgpu_ligero_param p_;
  lfgpu_ligero_prover* lp_ = nullptr;
};

template <class Field>
class GpuLigeroVerifier {
  using Elt = typename Field::Elt;

 public:
  explicit GpuLigeroVerifier(const Context& ctx) : c_(ctx) {}
  template <class CommitmentT, class TranscriptT>
  static void receive_commitment(const CommitmentT& com, TranscriptT& ts) {
    ts.write(com.root.data, 32);
  }
  // LigeroVerifier::verify (ligero_verifier.h:42-123); *why names the failing check with the reference's strings
  template <class ParamT, class CommitmentT, class ProofT, class TranscriptT, class LlT, class HashT, class LqcT>
  bool verify(const char** why, const ParamT& p, const CommitmentT& com, const ProofT& proof, TranscriptT& ts, size_t nl, size_t nllterm,
              const LlT llterm[], const HashT& hash_of_llterm, const Elt b[], const LqcT lqc[], const Field& F) const {
    const lfgpu_ligero_param q = detail::ligero_param_of<Field>(c_.get(), p);
    std::vector<uint8_t> wire;
    detail::com_proof_to_wire(proof, F, wire);
    detail::TranscriptHook<Field, TranscriptT> hook{&ts, &F, nullptr};
    const lfgpu_transcript_ops ops = hook.ops();
    int ok = 0;
    const char* reason = nullptr;
    if constexpr (field_id<Field>() == LFGPU_FIELD_P256) {
      check(c_.get(),
            lfgpu_ligero_verify256(c_.get(), &q, com.root.data, wire.data(), wire.size(), &ops, nl, nllterm, detail::llterm256_image(llterm),
                                   hash_of_llterm.bytes, b, detail::lqc_image(lqc), &ok, &reason),
            "lfgpu_ligero_verify256");
    } else {
      check(c_.get(),
            lfgpu_ligero_verify(c_.get(), field_id<Field>(), subfield_log_bits<Field>(), &q, com.root.data, wire.data(), wire.size(), &ops, nl,
                                nllterm, detail::llterm_image(llterm), hash_of_llterm.bytes, b, detail::lqc_image(lqc), &ok, &reason),
            "lfgpu_ligero_verify");
    }
    if (why) *why = reason;
    return ok != 0;
  }

 private:
  const Context& c_;
};

}  // namespace lfgpu
#endif  // LFGPU_ZK_ADAPTERS_H_
