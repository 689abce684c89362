// zk_proto.h -- the host-side ZK protocol layer, written once over a per-width policy P.
//
// zk.hip (GF(2^128) and Fp128, 16-byte elements) and zk256.hip (Fp256Base, 32-byte elements) each supply a policy and
// instantiate what is here.  Host control flow restated from the reference (no reference code is linked or copied):
//   RandomEngine::nat / choose         lib/random/random.h:57-105
//   ZkProver::fill_pad, setup_lqc      lib/zk/zk_prover.h:152-188, zk_common.h:149-160
//   ZkProver::prove                    lib/zk/zk_prover.h:98-149, ProverLayers::prove lib/sumcheck/prover_layers.h:106-183,320-344
//   ZkCommon::verifier_constraints     lib/zk/zk_common.h:49-136,406-439
//   LigeroProver::prove                lib/ligero/ligero_prover.h:84-146, inner_product_vector ligero_param.h:382-421
//   ZkProof::write / read              lib/zk/zk_proof.h:90-185,218-345
//   ZkVerifier::verify                 lib/zk/zk_verifier.h:68-94, LigeroVerifier::verify lib/ligero/ligero_verifier.h:42-270
//
// The Ligero halves of prove and verify stand on their own (ligero_prove, ligero_verify, com_proof_write / com_proof_read): the ZK
// functions call them, and so do lfgpu_ligero_prove / lfgpu_ligero_verify (zk.hip) for a caller's own statement.
//
// A policy is a plain struct.  Its host half (Wire16 / Wire32 below) is all that the transcript view, pad_layout,
// proof_write / proof_read (com_proof_write / com_proof_read) and inner_product_sparse use, so those run with no device context:
//   E, Field, kBytes, zero / is_zero / eq, to_bytes / of_bytes / sample, ts_write_elt / ts_write_array (how the transcript
//   hooks are called), and kSubfieldCodec: whether the wire format's two-byte subfield runs can occur (then also
//   two_byte_subfield / solve_subfield / of_subfield).
// build_constraints, prove and verify also call the device steps, which the .hip files add as static members:
//   Lig, kProveName, host_field, kDeferGh, eval_layer, sumcheck_layer, bind_gh_all (+ gh_enqueue / gh_read when kDeferGh),
//   eq_table, low_degree / dot / quadratic / open, verifier_ext.
// prove_batch (B statements in lock-step; both policies) also wants kProveBatchName, eval_layer_batch, sumcheck_layer_batch,
// eq_table_batch, ligero_prove_batch, ligero_open_batch and ligero_batch_switch (the A/B switch of the batched tail).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/lfgpu_zk.h"
#include "fp256.h"
#include "fs_crypto.h"
#include "hostfield.h"
#include "zkint.h"

// Everything below has internal linkage: each file that includes this header wants its own copy, and the library exports
// nothing from here.
namespace {
// ------------------------------------------------------------------ host field (FpGeneric over the P-256 prime)
struct F256 {
  elt32_t zero = e32_zero(), one, pts[3], invden[3], rsq;
  F256() {
    rsq = h256_rsq();
    one = h256_of_scalar(1);
    pts[0] = zero;  // poly_evaluation_points 0, 1, 2 (fp_generic.h:114-121)
    pts[1] = one;
    pts[2] = h256_of_scalar(2);
    for (int i = 0; i < 3; ++i) {
      elt32_t d = one;
      for (int j = 0; j < 3; ++j)
        if (j != i) d = fp256_mul(d, fp256_sub(pts[i], pts[j]));
      invden[i] = h256_inv(d);
    }
  }
  static elt32_t add(const elt32_t& a, const elt32_t& b) { return fp256_add(a, b); }
  static elt32_t sub(const elt32_t& a, const elt32_t& b) { return fp256_sub(a, b); }
  static elt32_t mul(const elt32_t& a, const elt32_t& b) { return fp256_mul(a, b); }
  // Poly<3>::eval_monomial (lib/algebra/poly.h:100-108)
  elt32_t eval_monomial(const elt32_t coef[3], const elt32_t& x) const { return add(mul(add(mul(coef[2], x), coef[1]), x), coef[0]); }
  // the quadratic through (pts[i], ev[i]) at x = Poly<3>::eval_lagrange (poly.h:72-98)
  elt32_t eval_lagrange(const elt32_t ev[3], const elt32_t& x) const {
    elt32_t acc = zero;
    for (int i = 0; i < 3; ++i) {
      elt32_t num = one;
      for (int j = 0; j < 3; ++j)
        if (j != i) num = mul(num, sub(x, pts[j]));
      acc = add(acc, mul(ev[i], mul(num, invden[i])));
    }
    return acc;
  }
};
}  // namespace

namespace zkp {
namespace {
constexpr size_t kMaxBindings = 40;  // Proof::kMaxBindings (lib/sumcheck/circuit.h:84)
constexpr size_t kMaxRunLen = (size_t)1 << 25, kMaxNumDigests = (size_t)1 << 25;  // zk_proof.h
inline size_t layer_size(size_t logw) { return 4 * logw + 3; }  // PadLayout::layer_size (zk_common.h:210-222)
inline size_t pad_size(const lfgpu_circuit* C) {
  size_t n = 0;
  for (const auto& l : C->layers) n += layer_size(l.logw);
  return n;
}
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// to_bytes_field / of_bytes_field / sample of the two 16-byte fields (lib/gf2k/gf2_128.h:168-190, lib/algebra/fp_generic.h:344-383)
inline void elt_to_bytes(int field, elt_t e, uint8_t out[16]) {
  if (field != LFGPU_FIELD_GF2_128) e = fp_from_mont(e);
  memcpy(out, &e, 16);
}
inline bool elt_of_bytes(int field, const uint8_t in[16], elt_t& e) {
  memcpy(&e, in, 16);
  if (field == LFGPU_FIELD_GF2_128) return true;  // every 128-bit string is an element
  if (!h_fp_fits(e)) return false;
  e = h_fp_to_mont(e);
  return true;
}
template <class Fill>
inline elt_t elt_sample(int field, Fill fill) {  // rejection sampling for Fp128 (exact_bits = 128: no masking)
  for (;;) {
    uint8_t b[16];
    fill(b, 16);
    elt_t e;
    if (elt_of_bytes(field, b, e)) return e;
  }
}

// subfield solver for the wire format (GF2_128::solve, lib/gf2k/gf2_128.h:496-508): echelon rows of beta
struct SubfieldSolver {
  struct Row {
    elt_t v;
    u32 comb;
    int pivot;
  };
  std::vector<Row> ech;  // REDUCED echelon form: a row's pivot bit is clear in every other row
  // table form of the same solve: the pivot bits of e, taken as two bytes, index the XOR of the rows (and of their combinations)
  // those bits select -- 2 lookups per element instead of a 16-step elimination (35 000 opened elements in an mdoc hash proof)
  elt_t ech_v[2][256];
  u32 ech_c[2][256];
  static int top_bit(elt_t v) { return v.hi ? 64 + (63 - __builtin_clzll(v.hi)) : v.lo ? 63 - __builtin_clzll(v.lo) : -1; }
  static bool bit_of(elt_t v, int j) { return j >= 64 ? (v.hi >> (j - 64)) & 1 : (v.lo >> j) & 1; }
  void build(const GfHostCtx* g) {
    ech.clear();
    for (unsigned i = 0; i < g->sub_bits; ++i) {
      elt_t v = g->beta[i];
      u32 comb = 1u << i;
      for (const auto& r : ech)
        if (bit_of(v, r.pivot)) {
          v = gf_add(v, r.v);
          comb ^= r.comb;
        }
      ech.push_back({v, comb, top_bit(v)});  // beta is a basis: v != 0
    }
    // back-substitute: every pivot bit survives in its own row only, so the pivot bits of an element ARE its elimination pattern
    for (size_t i = 0; i < ech.size(); ++i)
      for (size_t j = 0; j < ech.size(); ++j)
        if (j != i && bit_of(ech[j].v, ech[i].pivot)) {
          ech[j].v = gf_add(ech[j].v, ech[i].v);
          ech[j].comb ^= ech[i].comb;
        }
    for (int half = 0; half < 2; ++half)
      for (unsigned m = 0; m < 256; ++m) {
        elt_t v{0, 0};
        u32 cmb = 0;
        for (unsigned b = 0; b < 8; ++b) {
          const size_t r = 8 * half + b;
          if (((m >> b) & 1) && r < ech.size()) {
            v = gf_add(v, ech[r].v);
            cmb ^= ech[r].comb;
          }
        }
        ech_v[half][m] = v;
        ech_c[half][m] = cmb;
      }
  }
  // (residue, coordinates): residue == 0 iff e lies in the subfield, and then e = sum_i bit_i(u) beta_i
  std::pair<elt_t, u32> solve(elt_t e) const {
    if (ech.size() > 16) {  // (a 32-bit subfield: the plain elimination; the rows are reduced, the order does not matter)
      u32 u = 0;
      for (const auto& r : ech)
        if (bit_of(e, r.pivot)) {
          e = gf_add(e, r.v);
          u ^= r.comb;
        }
      return {e, u};
    }
    unsigned m = 0;
    for (size_t r = 0; r < ech.size(); ++r) m |= (unsigned)bit_of(e, ech[r].pivot) << r;
    const elt_t res = gf_add(e, gf_add(ech_v[0][m & 255], ech_v[1][m >> 8]));
    return {res, ech_c[0][m & 255] ^ ech_c[1][m >> 8]};
  }
};

// ------------------------------------------------------------------ the host halves of the two policies
struct Wire16 {  // GF(2^128) and Fp128; HostField dispatches on the field id
  using E = elt_t;
  using Field = HostField;
  static constexpr size_t kBytes = 16;
  int field = LFGPU_FIELD_GF2_128;
  const GfHostCtx* g = nullptr;         // GF(2^128): sub_tab, of_scalar by bytes (the reader)
  const SubfieldSolver* sub = nullptr;  // GF(2^128): in_subfield + coordinates (the writer)
  static E zero() { return elt_t{0, 0}; }
  static bool is_zero(const E& e) { return (e.lo | e.hi) == 0; }
  static bool eq(const E& a, const E& b) { return elt_eq(a, b); }
  void to_bytes(const E& e, uint8_t* out) const { elt_to_bytes(field, e, out); }
  bool of_bytes(const uint8_t* in, E& e) const { return elt_of_bytes(field, in, e); }
  template <class Fill>
  E sample(Fill fill) const { return elt_sample(field, fill); }
  // fill_pad's draws (stage_witness): use(draw), where draw() is RandomEngine::elt at the moment pad_layout asks for an element
  template <class Fill, class Use>
  size_t with_pad_draw(size_t, bool, Fill fill, Use use) const {
    return use([&] { return elt_sample(field, fill); });
  }
  void ts_write_elt(const lfgpu_transcript_ops* o, void* u, const uint8_t* b) const { o->write_elt(u, b); }
  void ts_write_array(const lfgpu_transcript_ops* o, void* u, const uint8_t* b, size_t n) const { o->write_elt_array(u, b, n); }
  // the elements as the transcript wants them, when that is their storage (GF(2^128)); else nullptr: convert one by one
  const uint8_t* raw_image(const E* e) const { return field == LFGPU_FIELD_GF2_128 ? (const uint8_t*)e : nullptr; }
  // subfield codec: GF(2^128) sends a subfield element as its kSubFieldBytes coordinate bytes (2 for GF2_128<4>, the ZK wire
  // format's; 4 for GF2_128<5>, which only the Ligero entry points serve); for Fp128 to/of_bytes_subfield == to/of_bytes_field
  static constexpr bool kSubfieldCodec = true;
  bool two_byte_subfield() const { return field == LFGPU_FIELD_GF2_128; }
  size_t subfield_bytes() const { return g->sub_bits / 8; }
  std::pair<E, u32> solve_subfield(const E& e) const { return sub->solve(e); }
  E of_subfield(const uint8_t* b) const {  // of_scalar(u) = sum_i bit_i(u) beta_i
    E e = gf_add(g->sub_tab[0][b[0]], g->sub_tab[1][b[1]]);
    for (size_t i = 2; i < subfield_bytes(); ++i) e = gf_add(e, g->sub_tab[i][b[i]]);
    return e;
  }
};

struct Wire32 {  // Fp256Base: every element is in the subfield, encoded at full width
  using E = elt32_t;
  using Field = F256;
  static constexpr size_t kBytes = 32;
  static E zero() { return e32_zero(); }
  static bool is_zero(const E& e) { return e32_is_zero(e); }
  static bool eq(const E& a, const E& b) { return e32_eq(a, b); }
  static void to_bytes(const E& e, uint8_t* out) { h256_to_bytes(e, out); }
  static bool of_bytes(const uint8_t* in, E& e) { return h256_of_bytes(in, e); }
  template <class Fill>
  static E sample(Fill fill) { return h256_sample(fill); }
  // fill_pad's draws (stage_witness): all ndraw elements first -- ONE bulk h256_sample_many, or under exact calls one call of 1
  // per element -- into a scrubbed vector, then use(draw), where draw() hands them out in order
  template <class Fill, class Use>
  static size_t with_pad_draw(size_t ndraw, bool exact, Fill fill, Use use) {
    std::vector<E> pads(ndraw);
    LF_SCRUB_ON_EXIT(pads);
    if (exact) for (auto& e : pads) h256_sample_many(&e, 1, fill);
    else h256_sample_many(pads.data(), ndraw, fill);
    size_t pd = 0;
    return use([&] { return pads[pd++]; });
  }
  static void ts_write_elt(const lfgpu_transcript_ops* o, void* u, const uint8_t* b) { o->write_elt_sized(u, b, 32); }
  static void ts_write_array(const lfgpu_transcript_ops* o, void* u, const uint8_t* b, size_t n) { o->write_elt_array_sized(u, b, n, 32); }
  static const uint8_t* raw_image(const E*) { return nullptr; }
  static constexpr bool kSubfieldCodec = false;
};

// ------------------------------------------------------------------ transcript view
// the caller's transcript seen through the hooks, plus the samplers built on RandomEngine::bytes
template <class P>
struct Ts {
  using E = typename P::E;
  const P* pol;
  const lfgpu_transcript_ops* o;
  void* u;
  void write_bytes(const uint8_t* d, size_t n) const { o->write_bytes(u, d, n); }
  void write_elt(const E& e) const {
    uint8_t b[P::kBytes];
    pol->to_bytes(e, b);
    pol->ts_write_elt(o, u, b);
  }
  void write_array(const E* e, size_t n) const {
    if (const uint8_t* raw = pol->raw_image(e)) return pol->ts_write_array(o, u, raw, n);
    std::vector<uint8_t> b(P::kBytes * (n ? n : 1));
    for (size_t i = 0; i < n; ++i) pol->to_bytes(e[i], &b[P::kBytes * i]);
    pol->ts_write_array(o, u, b.data(), n);
  }
  E elt() const {
    return pol->sample([&](uint8_t* b, size_t n) { o->gen_bytes(u, b, n); });
  }
  size_t nat(size_t n) const {  // RandomEngine::nat (lib/random/random.h:57-87): rejection sampling under a bit mask
    size_t l = 0, mask = 0;
    for (size_t nn = n; nn; nn >>= 8) ++l;
    while ((n & mask) != n) mask = (mask << 1) | 1;
    for (;;) {
      uint8_t b[8] = {0};
      o->gen_bytes(u, b, l);
      size_t r = 0;
      for (size_t i = 0; i < l; ++i) r |= (size_t)b[i] << (8 * i);
      r &= mask;
      if (r < n) return r;
    }
  }
  void choose(size_t n, size_t k, size_t* res) const {  // RandomEngine::choose (:89-105): partial Fisher-Yates
    std::vector<size_t> A(n);
    for (size_t i = 0; i < n; ++i) A[i] = i;
    for (size_t i = 0; i < k; ++i) {
      const size_t j = i + nat(n - i);
      std::swap(A[i], A[j]);
      res[i] = A[i];
    }
  }
};

// ------------------------------------------------------------------ proof-shaped data
template <class E>
struct LayerPad {  // Proof-shaped pad (zk_prover.h:152-188): hp[hand][2 round + {0, 1}] = {p(0), p(2)}, wc[2]
  std::vector<E> hp[2];
  E wc[2];
};
template <class E>
struct ComProof {  // LigeroProof: the write_com_proof section of the wire format
  std::vector<E> y_ldt, y_dot, y_q0, y_q2, req;
  std::vector<uint8_t> nonces, path;
  size_t npath = 0;
};
template <class E>
struct ProofBody : ComProof<E> {  // ZkProof: what ZkProof::write sends and ZkProof::read parses
  uint8_t root[32] = {0};
  std::vector<LayerPad<E>> sc;  // the padded (transmitted) sumcheck values
};
template <class P>
struct ProverState {  // what a prover keeps between commit, prove and proof_write
  using E = typename P::E;
  lfgpu_ligero_param param{};
  size_t npub = 0, n_witness = 0, pad_size = 0;
  std::vector<LayerPad<E>> pad;
  ProofBody<E> proof;
  std::vector<E> aux;  // ProofAux::bound_quad per layer
  std::vector<size_t> lqc;
  bool have_proof = false;
  mutable std::vector<uint8_t> wire;  // ZkProof::write bytes of the held proof (proof_write_cached fills it once)
  mutable bool wire_valid = false;
  double ms[6] = {0, 0, 0, 0, 0, 0};  // lfgpu_zk_timings: commit, prove, eval_circuit, sumcheck, constraints, Ligero
  void init(const lfgpu_circuit* C) {
    npub = C->info.npub_in;
    n_witness = C->info.ninputs - C->info.npub_in;
    pad_size = zkp::pad_size(C);
  }
  ~ProverState() {  // the host copies of the pads are secrets of the prover
    for (auto& L : pad) {
      for (auto& v : L.hp) std::fill(v.begin(), v.end(), P::zero());
      L.wc[0] = L.wc[1] = P::zero();
    }
  }
};

// setup_lqc (zk_common.h:149-160): lqc[3 ly + k] = claim_pad(k) of layer ly; returns the witness length.  With pad != nullptr
// also fill_pad (zk_prover.h:152-188, logc = 0): draws, per layer, (t0, t2) for hand 0 then hand 1 of every round, then wc0,
// wc1, and stores them and wc0 * wc1 behind the private inputs in Wv.
template <class P, class Draw>
size_t pad_layout(const typename P::Field& F, const lfgpu_circuit* C, size_t n_witness, std::vector<size_t>& lqc, Draw draw,
                  std::vector<LayerPad<typename P::E>>* pad, typename P::E* Wv) {
  const size_t nl = C->layers.size();
  if (pad) pad->assign(nl, {});
  lqc.assign(3 * nl, 0);
  size_t pi = n_witness;
  for (size_t ly = 0; ly < nl; ++ly) {
    const size_t logw = C->layers[ly].logw;
    if (pad) {
      auto& L = (*pad)[ly];
      L.hp[0].resize(2 * logw);
      L.hp[1].resize(2 * logw);
      size_t w = pi;
      for (size_t j = 0; j < logw; ++j)
        for (int h = 0; h < 2; ++h) {
          L.hp[h][2 * j] = draw();
          L.hp[h][2 * j + 1] = draw();
          Wv[w++] = L.hp[h][2 * j];
          Wv[w++] = L.hp[h][2 * j + 1];
        }
      L.wc[0] = draw();
      L.wc[1] = draw();
      Wv[w++] = L.wc[0];
      Wv[w++] = L.wc[1];
      Wv[w++] = F.mul(L.wc[0], L.wc[1]);
    }
    const size_t cp = pi + 4 * logw;
    lqc[3 * ly] = cp;
    lqc[3 * ly + 1] = cp + 1;
    lqc[3 * ly + 2] = cp + 2;
    pi += layer_size(logw);
  }
  return pi;
}
// The witness of ZkProver::commit (zk_prover.h:72-96) into Wv[param.nw]: the private inputs of h_W, then fill_pad's elements
// drawn from fill(bytes, n) the policy's way (with_pad_draw: every element but the computed wc0 * wc1 of each layer).  Returns
// pad_layout's length, which is param.nw.
template <class P, class Fill>
size_t stage_witness(const P& pol, const typename P::Field& F, const lfgpu_circuit* C, ProverState<P>& st, const void* h_W, bool rng_exact, Fill fill,
                     typename P::E* Wv) {
  memcpy(Wv, (const typename P::E*)h_W + st.npub, st.n_witness * sizeof(typename P::E));
  return pol.with_pad_draw(st.pad_size - C->layers.size(), rng_exact, fill,
                           [&](auto draw) { return pad_layout<P>(F, C, st.n_witness, st.lqc, draw, &st.pad, Wv); });
}

// ------------------------------------------------------------------ ZkProof::write / read
// write_com_proof (zk_proof.h:137-185), appended to o: the Ligero section, shared by ZkProof::write and lfgpu_ligero_prove
template <class P>
void com_proof_write(const P& pol, const ComProof<typename P::E>& pr, std::vector<uint8_t>& o) {
  using E = typename P::E;
  auto pute = [&](const E& e) {
    uint8_t b[P::kBytes];
    pol.to_bytes(e, b);
    o.insert(o.end(), b, b + P::kBytes);
  };
  auto putsz = [&](size_t g) {  // write_size: 4 bytes LE (zk_proof.h:211-216)
    for (int i = 0; i < 4; ++i) o.push_back((uint8_t)(g >> (8 * i)));
  };
  for (const E& e : pr.y_ldt) pute(e);
  for (const E& e : pr.y_dot) pute(e);
  for (const E& e : pr.y_q0) pute(e);
  for (const E& e : pr.y_q2) pute(e);
  o.insert(o.end(), pr.nonces.begin(), pr.nonces.end());
  // opened columns: alternating runs of full-field / subfield elements, run-length prefixed (:156-178).  GF(2^128): every
  // opened element is solved against the subfield basis ONCE (residue == 0 iff it lies in the subfield; the coordinates are
  // its kSubFieldBytes image: 2 bytes for GF2_128<4>, 4 for GF2_128<5>).  A prime field's elements all lie in the subfield: an
  // empty full-field run, then subfield runs.
  const size_t nreq_elts = pr.req.size();
  bool two = false;
  size_t sub_bytes = 2;
  std::vector<u32> sub_coord;
  std::vector<uint8_t> sub_flag;
  if constexpr (P::kSubfieldCodec) {
    if ((two = pol.two_byte_subfield())) {
      sub_bytes = pol.subfield_bytes();
      sub_coord.resize(nreq_elts);
      sub_flag.resize(nreq_elts);
      for (size_t i = 0; i < nreq_elts; ++i) {
        const auto r = pol.solve_subfield(pr.req[i]);
        sub_flag[i] = P::is_zero(r.first);
        sub_coord[i] = r.second;
      }
    }
  }
  o.reserve(o.size() + nreq_elts * P::kBytes + 32 * pr.npath + 64);
  size_t ci = 0;
  bool subfield_run = false;
  while (ci < nreq_elts) {
    size_t runlen = 0;
    if (two) {
      while (ci + runlen < nreq_elts && runlen < kMaxRunLen && (sub_flag[ci + runlen] != 0) == subfield_run) ++runlen;
    } else if (subfield_run) {
      runlen = std::min(nreq_elts - ci, kMaxRunLen);
    }
    putsz(runlen);
    for (size_t i = ci; i < ci + runlen; ++i) {
      if (subfield_run && two) {
        const u32 u = sub_coord[i];  // to_bytes_subfield: kSubFieldBytes LE
        for (size_t b = 0; b < sub_bytes; ++b) o.push_back((uint8_t)(u >> (8 * b)));
      } else {  // full-field run, or a prime field where to_bytes_subfield == to_bytes_field
        pute(pr.req[i]);
      }
    }
    ci += runlen;
    subfield_run = !subfield_run;
  }
  putsz(pr.npath);
  o.insert(o.end(), pr.path.begin(), pr.path.begin() + 32 * pr.npath);
}
template <class P>
void proof_write(const P& pol, const lfgpu_circuit* C, const ProofBody<typename P::E>& pr, std::vector<uint8_t>& o) {
  using E = typename P::E;
  o.clear();
  auto pute = [&](const E& e) {
    uint8_t b[P::kBytes];
    pol.to_bytes(e, b);
    o.insert(o.end(), b, b + P::kBytes);
  };
  o.insert(o.end(), pr.root, pr.root + 32);  // write_com
  for (size_t ly = 0; ly < pr.sc.size(); ++ly) {  // write_sc_proof: p(0) and p(2) of both hands per round, then wc
    const auto& L = pr.sc[ly];
    const size_t logw = C->layers[ly].logw;
    for (size_t wi = 0; wi < logw; ++wi)
      for (int k = 0; k < 2; ++k) {
        pute(L.hp[0][2 * wi + k]);
        pute(L.hp[1][2 * wi + k]);
      }
    pute(L.wc[0]);
    pute(L.wc[1]);
  }
  com_proof_write(pol, pr, o);
}

// lfgpu_zk_proof_write: serialised once per proof, the size query and the copy share the bytes
template <class P>
int proof_write_cached(lfgpu_ctx* c, const P& pol, const lfgpu_circuit* C, const ProverState<P>& st, uint8_t* buf, size_t cap, size_t* nbytes) {
  if (!st.have_proof) return lf_fail(c, LFGPU_ERR_ARG, "zk_proof_write: no proof");
  if (!st.wire_valid) {
    proof_write(pol, C, st.proof, st.wire);
    st.wire_valid = true;
  }
  *nbytes = st.wire.size();
  if (buf) {
    if (cap < st.wire.size()) return lf_fail(c, LFGPU_ERR_ARG, "zk_proof_write: buffer too small (%zu < %zu)", cap, st.wire.size());
    memcpy(buf, st.wire.data(), st.wire.size());
  }
  return LFGPU_OK;
}

// The cursor of the two readers below: what is left of the input, and whether an of_bytes_field failed (value >= p)
template <class P>
struct WireReader {
  const P& pol;
  const uint8_t* q;
  size_t left;
  bool bad = false;
  bool have(size_t n) const { return left >= n; }
  const uint8_t* next(size_t n) {
    const uint8_t* r = q;
    q += n;
    left -= n;
    return r;
  }
  typename P::E elt() {
    typename P::E e = P::zero();
    if (!pol.of_bytes(next(P::kBytes), e)) bad = true;
    return e;
  }
  size_t size4() {
    const uint8_t* b = next(4);
    return (size_t)b[0] | (size_t)b[1] << 8 | (size_t)b[2] << 16 | (size_t)b[3] << 24;
  }
};
// read_com_proof (zk_proof.h:262-345): the Ligero section at the cursor; false on underflow or inconsistent sizes (a bad element
// encoding is left in rd.bad).  Shared by ZkProof::read and lfgpu_ligero_verify.
template <class P>
bool com_proof_read(WireReader<P>& rd, const lfgpu_ligero_param& p, ComProof<typename P::E>& pr) {
  using E = typename P::E;
  constexpr size_t B = P::kBytes;
  const P& pol = rd.pol;
  auto vec = [&](std::vector<E>& v, size_t n) {
    if (!rd.have(n * B)) return false;
    v.resize(n);
    for (auto& e : v) e = rd.elt();
    return true;
  };
  if (!vec(pr.y_ldt, p.block) || !vec(pr.y_dot, p.dblock) || !vec(pr.y_q0, p.r) || !vec(pr.y_q2, p.dblock - p.block)) return false;
  if (!rd.have(p.nreq * 32)) return false;
  pr.nonces.assign(rd.q, rd.q + p.nreq * 32);
  rd.next(p.nreq * 32);
  const size_t total = p.nreq * p.nrow;
  bool two = false;
  size_t sub_bytes = 2;
  if constexpr (P::kSubfieldCodec) {
    if ((two = pol.two_byte_subfield())) sub_bytes = pol.subfield_bytes();
  }
  pr.req.assign(total, P::zero());
  size_t ci = 0;
  bool subfield_run = false;
  while (ci < total) {  // alternating full-field / subfield runs
    if (!rd.have(4)) return false;
    const size_t runlen = rd.size4();
    if (runlen >= kMaxRunLen || ci + runlen > total) return false;
    if (subfield_run && two) {
      if (!rd.have(runlen * sub_bytes)) return false;
      if constexpr (P::kSubfieldCodec)
        for (size_t i = ci; i < ci + runlen; ++i) pr.req[i] = pol.of_subfield(rd.next(sub_bytes));  // of_bytes_subfield
    } else {
      if (!rd.have(runlen * B)) return false;
      for (size_t i = ci; i < ci + runlen; ++i) pr.req[i] = rd.elt();
    }
    ci += runlen;
    subfield_run = !subfield_run;
  }
  if (!rd.have(4)) return false;
  const size_t sz = rd.size4();
  if (sz < p.nreq || sz >= kMaxNumDigests || sz > p.nreq * p.mc_pathlen || !rd.have(sz * 32)) return false;
  pr.npath = sz;
  pr.path.assign(rd.q, rd.q + sz * 32);
  rd.next(sz * 32);
  return true;
}

// ZkProof::read; false on underflow, inconsistent sizes or an element encoding >= p (the reference returns false as well)
template <class P>
bool proof_read(const P& pol, const lfgpu_circuit* C, const lfgpu_ligero_param& p, const uint8_t* buf, size_t len, ProofBody<typename P::E>& pr) {
  constexpr size_t B = P::kBytes;
  WireReader<P> rd{pol, buf, len};
  if (!rd.have(32)) return false;
  memcpy(pr.root, rd.next(32), 32);
  pr.sc.assign(C->layers.size(), {});
  for (size_t ly = 0; ly < C->layers.size(); ++ly) {
    const size_t logw = C->layers[ly].logw;
    if (!rd.have((logw * 4 + 2) * B)) return false;
    auto& L = pr.sc[ly];
    L.hp[0].resize(2 * logw);
    L.hp[1].resize(2 * logw);
    for (size_t wi = 0; wi < logw; ++wi)
      for (int k = 0; k < 2; ++k) {
        L.hp[0][2 * wi + k] = rd.elt();
        L.hp[1][2 * wi + k] = rd.elt();
      }
    L.wc[0] = rd.elt();
    L.wc[1] = rd.elt();
  }
  return com_proof_read(rd, p, pr) && !rd.bad;
}

// ------------------------------------------------------------------ verifier_constraints
// ZkCommon::verifier_constraints (lib/zk/zk_common.h:49-136) + input_constraint (:406-439), shared by the prover (aux = the
// bound quads the sumcheck prover recorded) and the verifier (aux = nullptr: Quad::bind_gh_all on the device).  Replays the
// verifier's side of the sumcheck on the transcript and returns the sparse rows of A (all but the dense private-input block
// of the last constraint) and b; the EQ table of the input constraint over all inputs is left in d_eq (device, the caller's).
template <class E>
struct LinTerm {
  size_t c, w;
  E k;
};
template <class E>
struct ConstraintSet {
  std::vector<LinTerm<E>> a;
  std::vector<E> b;  // one entry per constraint
  size_t n = 0;      // number of constraints; the dense one is n - 1
};
// What the EQ table of the input constraint is built from, for a caller that launches the tables of several statements at once
// (prove_finish_batch): build_constraints then stops in front of its EQ step, and input_constraint_b finishes the last entry of b
// once the public part of the table is back.
template <class E>
struct EqPending {
  std::vector<E> g0, g1;  // the last layer's challenges, logw each
  E alpha, wc0, wc1;
};
template <class P>
void input_constraint_b(const typename P::Field& F, const typename P::E& alpha, const typename P::E& wc0, const typename P::E& wc1, const typename P::E* eq_in,
                        const typename P::E* pub, size_t npub, ConstraintSet<typename P::E>& out) {
  typename P::E pub_binding = P::zero();
  for (size_t i = 0; i < npub; ++i) pub_binding = F.add(pub_binding, F.mul(eq_in[i], pub[i]));
  out.b.push_back(F.sub(F.add(wc0, F.mul(alpha, wc1)), pub_binding));
}
template <class P>
int build_constraints(lfgpu_ctx* c, const lfgpu_circuit* C, const typename P::Field& F, const Ts<P>& ts, const std::vector<LayerPad<typename P::E>>& proof,
                      const std::vector<typename P::E>* aux, const typename P::E* pub, typename P::E* d_eq, ConstraintSet<typename P::E>& out,
                      EqPending<typename P::E>* pend = nullptr) {
  using E = typename P::E;
  const lfgpu_circuit_info& I = C->info;
  const size_t nl = C->layers.size(), npub = I.npub_in;
  std::vector<E> G[2], gh[2];
  for (size_t i = 0; i < kMaxBindings; ++i) (void)ts.elt();  // begin_circuit: Q (unused for logc = 0), then G
  G[0].resize(kMaxBindings);
  for (size_t i = 0; i < kMaxBindings; ++i) G[0][i] = ts.elt();
  G[1] = G[0];
  size_t logv = I.logv, ci = 0, pi = I.ninputs - npub;
  E claims[2] = {P::zero(), P::zero()};
  std::vector<E> sym;
  struct Deferred {
    size_t ci, acp;  // constraint, position of its claim-pad terms in out.a
    E wc0, wc1;
  };
  std::vector<Deferred> deferred;
  // The verifier's bound quad feeds only ConstraintBuilder::finalize, never the transcript.  Where the policy can (kDeferGh)
  // and the layers' sums fit its mailbox, they are enqueued back to back and finalize runs for all layers after ONE read-back.
  bool defer = false;
  if constexpr (P::kDeferGh) defer = !aux && nl <= P::kGhBatchMax;
  for (size_t ly = 0; ly < nl; ++ly) {
    const auto& L = C->layers[ly];
    const size_t logw = L.logw;
    const E alpha = ts.elt(), beta = ts.elt();
    const size_t n = 3 + layer_size(logw);  // ovp_layer_size
    E known = P::zero();
    sym.assign(n, P::zero());
    auto axpy = [&](size_t var, const E& kv, const E& k) {  // Expression::axpy
      known = F.add(known, F.mul(k, kv));
      sym[var] = F.add(sym[var], k);
    };
    auto axmy = [&](size_t var, const E& kv, const E& k) {  // Expression::axmy
      known = F.sub(known, F.mul(k, kv));
      sym[var] = F.sub(sym[var], k);
    };
    axpy(0, claims[0], F.one);  // ConstraintBuilder::first
    axpy(1, claims[1], alpha);
    gh[0].assign(logw ? logw : 1, P::zero());
    gh[1].assign(logw ? logw : 1, P::zero());
    const auto& L_p = proof[ly];
    for (size_t rnd = 0; rnd < logw; ++rnd)
      for (int hand = 0; hand < 2; ++hand) {
        const size_t r = 2 * rnd + hand;
        const E t0e = L_p.hp[hand][2 * rnd], t2e = L_p.hp[hand][2 * rnd + 1];
        ts.write_elt(t0e);
        ts.write_elt(t2e);
        const E chal = ts.elt();
        gh[hand][rnd] = chal;
        E lag[3];  // dot_interpolation coefficients: p(chal) = sum_i lag[i] p(P_i)
        for (int i = 0; i < 3; ++i) {
          E num = F.one;
          for (int j = 0; j < 3; ++j)
            if (j != i) num = F.mul(num, F.sub(chal, F.pts[j]));
          lag[i] = F.mul(num, F.invden[i]);
        }
        axmy(3 + 2 * r, t0e, F.one);   // ConstraintBuilder::next: p(1) = claim - p(0)
        known = F.mul(known, lag[1]);  // scale
        for (auto& s : sym)
          if (!P::is_zero(s)) s = F.mul(s, lag[1]);
        axpy(3 + 2 * r, t0e, lag[0]);
        axpy(3 + 2 * r + 1, t2e, lag[2]);
      }
    // EQ[Q,C] QUAD[R,L] (Eq::eval with logc = 0 is 1): the prover's aux, or Quad::bind_gh_all on the device
    E eqq = P::zero();
    if (aux) {
      eqq = (*aux)[ly];
    } else if (defer) {
      if constexpr (P::kDeferGh) LF_TRY(P::gh_enqueue(c, L, logv, G[0].data(), G[1].data(), alpha, beta, gh[0].data(), gh[1].data(), ly));
    } else {
      LF_TRY(P::bind_gh_all(c, F, L, logv, G[0].data(), G[1].data(), alpha, beta, gh[0].data(), gh[1].data(), &eqq));
    }
    const size_t cp = 3 + 4 * logw;  // ConstraintBuilder::finalize
    const size_t a0 = out.a.size(), skip = ly == 0 ? 3 : 0;
    out.b.push_back(defer ? known : F.sub(F.mul(eqq, F.mul(L_p.wc[0], L_p.wc[1])), known));
    if (!defer) {
      sym[cp] = F.sub(sym[cp], F.mul(eqq, L_p.wc[1]));
      sym[cp + 1] = F.sub(sym[cp + 1], F.mul(eqq, L_p.wc[0]));
      sym[cp + 2] = F.sub(sym[cp + 2], eqq);
    }
    for (size_t i = skip; i < n; ++i) out.a.push_back({ci, pi + i - 3, sym[i]});
    if (defer) deferred.push_back({ci, a0 + cp - skip, L_p.wc[0], L_p.wc[1]});
    ++ci;
    ts.write_array(L_p.wc, 2);
    claims[0] = L_p.wc[0];
    claims[1] = L_p.wc[1];
    for (int h = 0; h < 2; ++h) {
      G[h].assign(kMaxBindings, P::zero());
      for (size_t r = 0; r < logw; ++r) G[h][r] = gh[h][r];
    }
    logv = logw;
    pi += layer_size(logw);
  }
  if constexpr (P::kDeferGh) {
    if (!deferred.empty()) {  // the layers' bind_gh_all sums: one read-back, then finalize each layer
      std::vector<E> sums;
      LF_TRY(P::gh_read(c, F, nl, sums));
      for (const Deferred& d : deferred) {
        const E eqq = sums[d.ci];
        out.b[d.ci] = F.sub(F.mul(eqq, F.mul(d.wc0, d.wc1)), out.b[d.ci]);  // b held `known` so far
        out.a[d.acp].k = F.sub(out.a[d.acp].k, F.mul(eqq, d.wc1));
        out.a[d.acp + 1].k = F.sub(out.a[d.acp + 1].k, F.mul(eqq, d.wc0));
        out.a[d.acp + 2].k = F.sub(out.a[d.acp + 2].k, eqq);
      }
    }
  }
  const E alpha = ts.elt();
  out.a.push_back({ci, pi - 3, F.sub(P::zero(), F.one)});  // input_constraint: -1, -alpha on the input layer's claim pads
  out.a.push_back({ci, pi - 2, F.sub(P::zero(), alpha)});
  out.n = ci + 1;
  // EQ(g0, i) + alpha EQ(g1, i) over the inputs on the device: the public part is folded into b, the private part is the
  // dense block of A
  const auto& L_p = proof[nl - 1];
  if (pend) {  // the caller builds the table (and nothing of this statement has been launched)
    pend->g0 = gh[0];
    pend->g1 = gh[1];
    pend->alpha = alpha;
    pend->wc0 = L_p.wc[0];
    pend->wc1 = L_p.wc[1];
    return LFGPU_OK;
  }
  std::vector<E> eq_in(npub ? npub : 1, P::zero());
  LF_TRY(P::eq_table(c, F, C->layers[nl - 1].logw, I.ninputs, gh[0].data(), gh[1].data(), alpha, d_eq, npub, eq_in.data()));
  input_constraint_b<P>(F, alpha, L_p.wc[0], L_p.wc[1], eq_in.data(), pub, npub, out);
  return LFGPU_OK;
}

// LigeroCommon::inner_product_vector (lib/ligero/ligero_param.h:382-421), host share: the sparse terms of A[nwqrow][w]
// -- the linear constraints' terms times alphal and the quadratic copy constraints (A[copy] += aq, A[original] -= aq) --
// as (flat index, value) pairs, sorted with duplicates folded.  The dense private-input block alphal[n-1] * EQ[npub + w]
// is built on the device; the sums commute, so the result is the reference's A.
template <class P>
void inner_product_sparse(const typename P::Field& F, const lfgpu_ligero_param& p, const std::vector<LinTerm<typename P::E>>& a,
                          const std::vector<typename P::E>& alphal, const std::vector<size_t>& lqc, const std::vector<typename P::E>& alphaq,
                          std::vector<uint64_t>& idx, std::vector<typename P::E>& val) {
  using E = typename P::E;
  std::vector<std::pair<uint64_t, E>> t;
  t.reserve(a.size() + 6 * p.nq);
  for (const LinTerm<E>& l : a) t.emplace_back((uint64_t)l.w, F.mul(l.k, alphal[l.c]));
  const size_t base = p.nwrow * p.w;
  const size_t Ax = base, Ay = base + p.nqtriples * p.w, Az = base + 2 * p.nqtriples * p.w;
  for (size_t iw = 0; iw < p.nq; ++iw) {
    const size_t off[3] = {Ax + iw, Ay + iw, Az + iw};
    for (int j = 0; j < 3; ++j) {
      const E aq = alphaq[3 * iw + j];
      t.emplace_back((uint64_t)off[j], aq);
      t.emplace_back((uint64_t)lqc[3 * iw + j], F.sub(P::zero(), aq));
    }
  }
  std::stable_sort(t.begin(), t.end(), [](const std::pair<uint64_t, E>& x, const std::pair<uint64_t, E>& y) { return x.first < y.first; });
  idx.clear();
  val.clear();
  for (const auto& e : t) {
    if (!idx.empty() && idx.back() == e.first) val.back() = F.add(val.back(), e.second);
    else {
      idx.push_back(e.first);
      val.push_back(e.second);
    }
  }
}

// ------------------------------------------------------------------ LigeroProver::prove / LigeroVerifier::verify
// The Ligero halves of ZkProver::prove and ZkVerifier::verify, also the whole of lfgpu_ligero_prove / lfgpu_ligero_verify.  What
// differs between the two callers is how the matrix A of inner_product_vector reaches the device (ZK: a dense EQ block on the
// device + host-folded sparse terms; Ligero entry points: the caller's term list), so that step is the caller's.
//
// LigeroProver::prove (ligero_prover.h:84-146) on the committed prover lp: challenges, the three row combinations, the y writes,
// choose and the opening.  dot(alphal, alphaq, y_dot): the caller's dot proof (it may stamp tq[2] where its host share ends).
// tq[6]: time stamps for the caller's verbose line.
template <class P, class Dot>
int ligero_prove(const lfgpu_ligero_param& p, typename P::Lig* lp, const Ts<P>& ts, const uint8_t hash_of_A[32], size_t nl, Dot dot,
                 ComProof<typename P::E>& pr, double tq[6]) {
  using E = typename P::E;
  ts.write_bytes(hash_of_A, 32);
  std::vector<E> u_ldt(p.nwqrow);
  for (auto& e : u_ldt) e = ts.elt();
  pr.y_ldt.assign(p.block, P::zero());
  tq[0] = now_ms();
  LF_TRY(P::low_degree(lp, u_ldt.data(), pr.y_ldt.data()));
  tq[1] = now_ms();
  std::vector<E> alphal(nl), alphaq(3 * p.nq);
  for (auto& e : alphal) e = ts.elt();
  for (auto& e : alphaq) e = ts.elt();
  pr.y_dot.assign(p.dblock, P::zero());
  tq[2] = now_ms();
  LF_TRY(dot(alphal, alphaq, pr.y_dot.data()));
  tq[3] = now_ms();
  std::vector<E> u_quad(p.nqtriples ? p.nqtriples : 1);
  for (size_t i = 0; i < p.nqtriples; ++i) u_quad[i] = ts.elt();
  pr.y_q0.assign(p.r, P::zero());
  pr.y_q2.assign(p.dblock - p.block, P::zero());
  LF_TRY(P::quadratic(lp, u_quad.data(), pr.y_q0.data(), pr.y_q2.data()));
  tq[4] = now_ms();
  ts.write_array(pr.y_ldt.data(), pr.y_ldt.size());
  ts.write_array(pr.y_dot.data(), pr.y_dot.size());
  ts.write_array(pr.y_q0.data(), pr.y_q0.size());
  ts.write_array(pr.y_q2.data(), pr.y_q2.size());
  std::vector<size_t> idx(p.nreq);
  ts.choose(p.block_ext, p.nreq, idx.data());
  pr.req.assign(p.nrow * p.nreq, P::zero());
  pr.nonces.assign(p.nreq * 32, 0);
  const size_t cap = p.nreq * p.mc_pathlen + 1;
  pr.path.assign(cap * 32, 0);
  LF_TRY(P::open(lp, idx.data(), pr.req.data(), pr.nonces.data(), pr.path.data(), cap, &pr.npath));
  tq[5] = now_ms();
  return LFGPU_OK;
}

// the verdicts of the verifiers: the reference's strings (lib/ligero/ligero_verifier.h:90-130) and ours for a proof that ZkProof::read refuses
enum { kWhyOk = 0, kWhyParse, kWhyMerkle, kWhyLowDegree, kWhyDot, kWhyDotValue, kWhyQuadratic };
inline const char* why_string(int w) {
  static const char* kWhy[] = {"ok", "proof does not parse", "merkle_check failed", "low_degree_check failed", "dot_check failed",
                               "wrong dot product", "quadratic_check failed"};
  return kWhy[w];
}
// LigeroVerifier::verify (ligero_verifier.h:42-123) over a parsed proof, the root already in the transcript: challenges, the Merkle
// check, then the three column checks and the value of the inner product against b[nl].  ext_fn(alphal, alphaq, idx, out): the
// caller's device step -- out[row][j] for the rows [0^r | A_i] (i < nwqrow) and then y_ldt, y_dot, y_quad, Reed-Solomon-extended, at
// the opened columns idx[j].  *why: the first failing check (kWhy...).  tv[3], tv[4]: time stamps after the Merkle check and the
// device step.
template <class P, class Ext>
int ligero_verify(const P& pol, const typename P::Field& F, const lfgpu_ligero_param& p, const uint8_t root[32], const ComProof<typename P::E>& pr,
                  const Ts<P>& ts, const uint8_t hash_of_A[32], size_t nl, const typename P::E* b, Ext ext_fn, int* why, double tv[6]) {
  using E = typename P::E;
  ts.write_bytes(hash_of_A, 32);
  std::vector<E> u_ldt(p.nwqrow), alphal(nl), alphaq(3 * p.nq), u_quad(p.nqtriples ? p.nqtriples : 1);
  for (auto& e : u_ldt) e = ts.elt();
  for (auto& e : alphal) e = ts.elt();
  for (auto& e : alphaq) e = ts.elt();
  for (size_t i = 0; i < p.nqtriples; ++i) u_quad[i] = ts.elt();
  ts.write_array(pr.y_ldt.data(), pr.y_ldt.size());
  ts.write_array(pr.y_dot.data(), pr.y_dot.size());
  ts.write_array(pr.y_q0.data(), pr.y_q0.size());
  ts.write_array(pr.y_q2.data(), pr.y_q2.size());
  std::vector<size_t> idx(p.nreq);
  ts.choose(p.block_ext, p.nreq, idx.data());
  auto req_at = [&](size_t i, size_t j) -> const E& { return pr.req[i * p.nreq + j]; };
  auto fail = [&](int w) {
    *why = w;
    return LFGPU_OK;
  };

  {  // merkle_check: leaf r = SHA-256(nonce_r || column r of the opening)
    std::vector<uint8_t> leaves(p.nreq * 32);
    for (size_t r = 0; r < p.nreq; ++r) {
      Sha256 s;
      s.update(&pr.nonces[32 * r], 32);
      for (size_t i = 0; i < p.nrow; ++i) {
        uint8_t eb[P::kBytes];
        pol.to_bytes(req_at(i, r), eb);
        s.update(eb, P::kBytes);
      }
      s.digest(&leaves[32 * r]);
    }
    if (!lf_merkle_verify(p.block_ext, root, pr.path.data(), pr.npath, leaves.data(), idx.data(), p.nreq)) return fail(kWhyMerkle);
  }
  tv[3] = now_ms();

  // device: rows [0, nwqrow) = [0^r | A_i] extended block -> block_enc, rows nwqrow.. = y_ldt, y_dot, y_quad; ext = their
  // opened columns
  std::vector<E> ext;
  LF_TRY(ext_fn(alphal, alphaq, idx.data(), ext));
  auto ext_at = [&](size_t row, size_t j) -> const E& { return ext[row * p.nreq + j]; };
  tv[4] = now_ms();

  for (size_t j = 0; j < p.nreq; ++j) {  // low_degree_check
    E yc = req_at(p.ildt, j);
    for (size_t i = 0; i < p.nwqrow; ++i) yc = F.add(yc, F.mul(u_ldt[i], req_at(i + p.iw, j)));
    if (!P::eq(yc, ext_at(p.nwqrow, j))) return fail(kWhyLowDegree);
  }
  for (size_t j = 0; j < p.nreq; ++j) {  // dot_check
    E yc = req_at(p.idot, j);
    for (size_t i = 0; i < p.nwqrow; ++i) yc = F.add(yc, F.mul(ext_at(i, j), req_at(i + p.iw, j)));
    if (!P::eq(yc, ext_at(p.nwqrow + 1, j))) return fail(kWhyDot);
  }
  {  // the putative value of the inner product
    E want = P::zero(), got = P::zero();
    for (size_t k = 0; k < nl; ++k) want = F.add(want, F.mul(b[k], alphal[k]));
    for (size_t j = 0; j < p.w; ++j) got = F.add(got, pr.y_dot[p.r + j]);
    if (!P::eq(want, got)) return fail(kWhyDotValue);
  }
  {  // quadratic_check
    const size_t iqx = p.iq, iqy = iqx + p.nqtriples, iqz = iqy + p.nqtriples;
    for (size_t j = 0; j < p.nreq; ++j) {
      E yc = req_at(p.iquad, j);
      for (size_t i = 0; i < p.nqtriples; ++i) {
        const E tmp = F.sub(req_at(iqz + i, j), F.mul(req_at(iqx + i, j), req_at(iqy + i, j)));  // z - x*y
        yc = F.add(yc, F.mul(u_quad[i], tmp));
      }
      if (!P::eq(yc, ext_at(p.nwqrow + 2, j))) return fail(kWhyQuadratic);
    }
  }
  return fail(kWhyOk);
}

// initialize_sumcheck_fiat_shamir (zk_common.h:163-180)
template <class P>
void fs_init(const Ts<P>& ts, const lfgpu_circuit* C, const typename P::E* pub) {
  ts.write_bytes(C->info.id, 32);
  for (size_t i = 0; i < C->info.npub_in; ++i) ts.write_elt(pub[i]);
  ts.write_elt(P::zero());
  ts.write_bytes(C->zeros->data(), C->info.nterms);
}

// ------------------------------------------------------------------ ZkProver::prove
template <class P>
struct RoundCtx {  // round_h of the padded prover (prover_layers.h:320-329): transmit poly - pad
  const typename P::Field* F;
  const Ts<P>* tst;
  const LayerPad<typename P::E>* pad;
  LayerPad<typename P::E>* out;
};
template <class P>
void round_cb(void* user, size_t hand, size_t rnd, const typename P::E ev[3], typename P::E* chal) {
  RoundCtx<P>* r = (RoundCtx<P>*)user;
  const typename P::E t0 = r->F->sub(ev[0], r->pad->hp[hand][2 * rnd]), t2 = r->F->sub(ev[2], r->pad->hp[hand][2 * rnd + 1]);
  r->out->hp[hand][2 * rnd] = t0;
  r->out->hp[hand][2 * rnd + 1] = t2;
  r->tst->write_elt(t0);
  r->tst->write_elt(t2);
  *chal = r->tst->elt();
}

// ---- the phases of prove: evaluation + fs_init, padded sumcheck, constraints + Ligero prove.  prove (one statement) and
// prove_batch (B statements in lock-step) are both written over the pieces below; only the device calls differ.
struct CloneGuard {  // the copy of the transcript that the sumcheck prover runs on (zk_prover.h:117-124)
  const lfgpu_transcript_ops* o;
  void* u;
  ~CloneGuard() {
    if (u) o->free_clone(u);
  }
};
// eval_circuit's verdict: no assert-zero term fired and every output is zero (prover_layers.h:52-104, zk_prover.h:104-112)
template <class P>
bool witness_ok(const typename P::E* V, size_t nv, int failed) {
  if (failed) return false;  // an assert-zero term is non-zero: eval_circuit returns nullptr
  for (size_t i = 0; i < nv; ++i)
    if (!P::is_zero(V[i])) return false;  // "V->v_[i] != F.zero()"
  return true;
}
template <class P>
struct ScRun {  // what the padded sumcheck of one statement carries from layer to layer (ProverLayers::prove with pad)
  using E = typename P::E;
  std::vector<E> G[2];
  E WC[2] = {P::zero(), P::zero()};
  size_t logv = 0;
};
template <class P>
void sc_begin(const Ts<P>& tst, const lfgpu_circuit* C, ProverState<P>& st, ScRun<P>& run) {
  const size_t nl = C->layers.size();
  st.proof.sc.assign(nl, {});
  st.aux.assign(nl, P::zero());
  for (size_t i = 0; i < kMaxBindings; ++i) (void)tst.elt();  // begin_circuit: Q then G (transcript_sumcheck.h:49-52)
  run.G[0].resize(kMaxBindings);
  for (size_t i = 0; i < kMaxBindings; ++i) run.G[0][i] = tst.elt();
  run.G[1] = run.G[0];
  run.logv = C->info.logv;
  run.WC[0] = run.WC[1] = P::zero();
}
// a layer's challenges alpha and beta, and the round context of its (hand, round) callbacks
template <class P>
RoundCtx<P> sc_layer_open(const typename P::Field& F, const Ts<P>& tst, ProverState<P>& st, size_t ly, size_t logw, typename P::E* alpha,
                          typename P::E* beta) {
  *alpha = tst.elt();
  *beta = tst.elt();
  auto& S = st.proof.sc[ly];
  S.hp[0].resize(2 * logw);
  S.hp[1].resize(2 * logw);
  return RoundCtx<P>{&F, &tst, &st.pad[ly], &S};
}
// end_layer (prover_layers.h:331-344): transmit wc - pad; the claims and the binding of the next layer
template <class P>
void sc_layer_close(const typename P::Field& F, const Ts<P>& tst, ProverState<P>& st, size_t ly, size_t logw, const typename P::E wc_out[2],
                    const typename P::E& bq, const typename P::E* gout /*[2][logw]*/, ScRun<P>& run) {
  auto& S = st.proof.sc[ly];
  S.wc[0] = F.sub(wc_out[0], st.pad[ly].wc[0]);
  S.wc[1] = F.sub(wc_out[1], st.pad[ly].wc[1]);
  tst.write_array(S.wc, 2);
  st.aux[ly] = bq;
  run.WC[0] = wc_out[0];
  run.WC[1] = wc_out[1];
  for (int h = 0; h < 2; ++h) {
    run.G[h].assign(kMaxBindings, P::zero());
    for (size_t r = 0; r < logw; ++r) run.G[h][r] = gout[h * logw + r];
  }
  run.logv = logw;
}
template <class P, class EqTable>
int prove_finish(lfgpu_ctx* c, const lfgpu_circuit* C, const P& pol, const typename P::Field& F, ProverState<P>& st, typename P::Lig* lp, EqTable eq_table,
                 const typename P::E* W, const Ts<P>& ts);

// d_in: the layers' inputs (eval_circuit leaves them resident for the sumcheck), d_V / h_V: the circuit outputs on the device
// and pinned (h_V: nv elements, then the assert-zero flag), eq_table(E** d_eq): room for the EQ table over the inputs (valid
// until lp's dot proof has run), asked for when the constraints are built.  *ok = 0 when the witness does not satisfy the
// circuit.
template <class P, class EqTable>
int prove(lfgpu_ctx* c, const lfgpu_circuit* C, const P& pol, ProverState<P>& st, typename P::Lig* lp, void* const* d_in, void* d_V, void* h_V,
          EqTable eq_table, const void* h_W, const lfgpu_transcript_ops* tso, int* ok) {
  using E = typename P::E;
  constexpr size_t B = P::kBytes;
  const double t_start = now_ms();
  const typename P::Field F = pol.host_field(c);
  const lfgpu_circuit_info& I = C->info;
  const size_t nl = C->layers.size();
  const E* W = (const E*)h_W;
  const Ts<P> ts{&pol, tso, tso->user};
  *ok = 0;
  st.have_proof = false;
  st.wire_valid = false;
  LF_HIP(c, hipSetDevice(c->device));

  // eval_circuit (prover_layers.h:52-104): layer inputs stay resident for the sumcheck.  The device works through all
  // layers back to back (assert-zero failures and the outputs are read once at the end) while the host hashes the
  // Fiat-Shamir preamble below -- SHA-256 over nterms zero bytes is sequential host work the reference's transcript
  // format fixes, and the evaluation does not depend on it.
  double t0 = now_ms();
  const E* V = (const E*)h_V;
  const int* failed = (const int*)((const uint8_t*)h_V + I.nv * B);
  {
    LF_HIP(c, hipMemcpyAsync(d_in[nl - 1], W, I.ninputs * B, hipMemcpyHostToDevice, c->stream));
    int* d_fail = (int*)((uint8_t*)c->mailbox_d + 128);
    LF_HIP(c, hipMemsetAsync(d_fail, 0, 4, c->stream));
    for (size_t l = nl; l-- > 0;) LF_TRY(P::eval_layer(C->layers[l].q, d_in[l], l ? d_in[l - 1] : d_V, d_fail));
    LF_HIP(c, hipMemcpyAsync(h_V, d_V, I.nv * B, hipMemcpyDeviceToHost, c->stream));
    LF_HIP(c, hipMemcpyAsync((uint8_t*)h_V + I.nv * B, d_fail, 4, hipMemcpyDeviceToHost, c->stream));
  }
  const double t_enq = now_ms() - t0;

  fs_init(ts, C, W);
  void* cl = tso->clone(tso->user);
  if (!cl) {
    (void)hipStreamSynchronize(c->stream);
    return lf_fail(c, LFGPU_ERR_NOMEM, "%s: transcript clone", P::kProveName);
  }
  CloneGuard cg{tso, cl};
  const Ts<P> tst{&pol, tso, cl};

  t0 = now_ms();
  LF_HIP(c, hipStreamSynchronize(c->stream));
  if (!witness_ok<P>(V, I.nv, *failed)) return LFGPU_OK;
  st.ms[2] = t_enq + now_ms() - t0;  // what the evaluation adds to the wall time: enqueue + the wait left after the hashing

  // padded sumcheck (ProverLayers::prove with pad, transcript copy tst)
  t0 = now_ms();
  ScRun<P> run;
  sc_begin<P>(tst, C, st, run);
  std::vector<E> gout;
  for (size_t ly = 0; ly < nl; ++ly) {
    const auto& L = C->layers[ly];
    E alpha, beta;
    RoundCtx<P> rc = sc_layer_open<P>(F, tst, st, ly, L.logw, &alpha, &beta);
    gout.assign(2 * L.logw + 1, P::zero());
    E wc_out[2], bq;
    LF_TRY(P::sumcheck_layer(L.q, F, run.logv, run.G[0].data(), run.G[1].data(), alpha, beta, L.logw, L.nw, d_in[ly], run.WC, round_cb<P>, &rc, wc_out,
                             gout.data(), &bq));
    sc_layer_close<P>(F, tst, st, ly, L.logw, wc_out, bq, gout.data(), run);
  }
  st.ms[3] = now_ms() - t0;

  LF_TRY(prove_finish<P>(c, C, pol, F, st, lp, eq_table, W, ts));
  st.ms[1] = now_ms() - t_start;
  *ok = 1;
  return LFGPU_OK;
}

// verifier_constraints with aux, then LigeroProver::prove, on the ORIGINAL transcript; the proof is then held by st
template <class P, class EqTable>
int prove_finish(lfgpu_ctx* c, const lfgpu_circuit* C, const P& pol, const typename P::Field& F, ProverState<P>& st, typename P::Lig* lp, EqTable eq_table,
                 const typename P::E* W, const Ts<P>& ts) {
  using E = typename P::E;
  (void)pol;
  ProofBody<E>& pr = st.proof;
  // verifier_constraints with aux (zk_common.h:49-136): replay the verifier symbolically on the ORIGINAL transcript
  double t0 = now_ms();
  E* d_eq = nullptr;
  LF_TRY(eq_table(&d_eq));
  ConstraintSet<E> cs;
  LF_TRY(build_constraints<P>(c, C, F, ts, pr.sc, &st.aux, W, d_eq, cs));
  const lfgpu_ligero_param& p = st.param;
  st.ms[4] = now_ms() - t0;

  // LigeroProver::prove (ligero_prover.h:84-146): A = the dense private-input block (the EQ table, on the device) + the sparse terms
  t0 = now_ms();
  {
    const uint8_t hash_of_A[32] = {0xde, 0xad, 0xbe, 0xef};  // zk_prover.h:143
    static const bool verbose = getenv("LFGPU_VERBOSE") != nullptr;
    double tq[6] = {0, 0, 0, 0, 0, 0};
    auto dot = [&](const std::vector<E>& alphal, const std::vector<E>& alphaq, E* y_dot) {
      std::vector<uint64_t> a_idx;
      std::vector<E> a_val;
      inner_product_sparse<P>(F, p, cs.a, alphal, st.lqc, alphaq, a_idx, a_val);
      tq[2] = now_ms();
      return P::dot(lp, d_eq + st.npub, st.n_witness, alphal[cs.n - 1], a_idx.data(), a_val.data(), a_idx.size(), y_dot);
    };
    LF_TRY(ligero_prove<P>(p, lp, ts, hash_of_A, cs.n, dot, pr, tq));
    if (verbose)
      fprintf(stderr, "lfgpu zk ligero_prove: ldt %.2f ms | sparse terms of A %.2f | dot %.2f | quad %.2f | challenges+open %.2f\n", tq[1] - tq[0],
              tq[2] - tq[1], tq[3] - tq[2], tq[4] - tq[3], tq[5] - tq[4]);
  }
  st.ms[5] = now_ms() - t0;
  st.have_proof = true;
  return LFGPU_OK;
}

// ------------------------------------------------------------------ B statements of one circuit in lock-step
// The device buffers of a batch (the caller's; nothing is allocated here): per layer nb_max input slabs at stride ldw[l]
// elements, the outputs at stride ldv, one assert-zero flag per statement, the pinned read-back (nb_max * ldv elements,
// then nb_max flags), and nb_max EQ tables over the inputs at a stride of ninputs elements (prove_finish_batch).
struct BatchBufs {
  void* const* d_in;
  const size_t* ldw;
  void* d_V;
  size_t ldv;
  int* d_fail;
  void* h_V;
  size_t nb_max;
  void* d_eq;
};
template <class P>
void round_batch_cb(void* user, size_t hand, size_t rnd, size_t nb, const typename P::E (*ev)[3], typename P::E* chal) {
  RoundCtx<P>* r = (RoundCtx<P>*)user;
  for (size_t b = 0; b < nb; ++b) round_cb<P>(&r[b], hand, rnd, ev[b], &chal[b]);
}
// prove_finish for the statements sel[0 .. m) of a batch (those with a good witness) with the device work of all of them in
// three chains: ONE EQ table launch (statement g's table at bb.d_eq + g * ninputs, its public part read back once), ONE
// lfgpu_ligero_prove_batch, ONE lfgpu_ligero_open_batch.  Per statement the transcript sees exactly what prove_finish shows
// it, in the same order: the device calls of the single path lie between draws and never touch the transcript.
// ms: {constraints, Ligero prove} of the whole batch.
template <class P>
int prove_finish_batch(lfgpu_ctx* c, const lfgpu_circuit* C, const typename P::Field& F, ProverState<P>* const* st, typename P::Lig* const* lp,
                       const BatchBufs& bb, const std::vector<size_t>& sel, const void* const* h_W, const std::vector<Ts<P>>& ts, double ms[2]) {
  using E = typename P::E;
  const lfgpu_circuit_info& I = C->info;
  const size_t m = sel.size(), nl = C->layers.size(), npub = I.npub_in, logn = C->layers[nl - 1].logw;
  const lfgpu_ligero_param& p = st[sel[0]]->param;
  // verifier_constraints with aux per statement on its ORIGINAL transcript (host only), then the EQ tables of all statements
  double t0 = now_ms();
  std::vector<ConstraintSet<E>> cs(m);
  std::vector<EqPending<E>> pend(m);
  for (size_t g = 0; g < m; ++g) {
    const size_t b = sel[g];
    LF_TRY(build_constraints<P>(c, C, F, ts[b], st[b]->proof.sc, &st[b]->aux, (const E*)h_W[b], nullptr, cs[g], &pend[g]));
  }
  E* const d_eq = (E*)bb.d_eq;
  {
    std::vector<E> G0(m * logn + 1, P::zero()), G1(m * logn + 1, P::zero()), al(m), eq_in(m * npub + 1, P::zero());
    for (size_t g = 0; g < m; ++g) {
      for (size_t l = 0; l < logn; ++l) {
        G0[g * logn + l] = pend[g].g0[l];
        G1[g * logn + l] = pend[g].g1[l];
      }
      al[g] = pend[g].alpha;
    }
    LF_TRY(P::eq_table_batch(c, F, m, logn, I.ninputs, G0.data(), G1.data(), al.data(), d_eq, npub, eq_in.data()));
    for (size_t g = 0; g < m; ++g)
      input_constraint_b<P>(F, pend[g].alpha, pend[g].wc0, pend[g].wc1, eq_in.data() + g * npub, (const E*)h_W[sel[g]], npub, cs[g]);
  }
  ms[0] = now_ms() - t0;

  // LigeroProver::prove (ligero_prover.h:84-146): the draws of every statement, then the device work of all of them
  t0 = now_ms();
  const size_t nqt = p.nqtriples, ymid = p.dblock - p.block;
  std::vector<E> u_ldt(m * p.nwqrow + 1, P::zero()), u_quad(m * nqt + 1, P::zero()), scale(m);
  std::vector<std::vector<uint64_t>> a_idx(m);
  std::vector<std::vector<E>> a_val(m);
  std::vector<const uint64_t*> pi(m);
  std::vector<const E*> pv(m), pdense(m);
  std::vector<size_t> nsp(m);
  std::vector<typename P::Lig*> lps(m);
  for (size_t g = 0; g < m; ++g) {
    const size_t b = sel[g];
    const uint8_t hash_of_A[32] = {0xde, 0xad, 0xbe, 0xef};  // zk_prover.h:143
    ts[b].write_bytes(hash_of_A, 32);
    for (size_t i = 0; i < p.nwqrow; ++i) u_ldt[g * p.nwqrow + i] = ts[b].elt();
    std::vector<E> alphal(cs[g].n), alphaq(3 * p.nq);
    for (auto& e : alphal) e = ts[b].elt();
    for (auto& e : alphaq) e = ts[b].elt();
    inner_product_sparse<P>(F, p, cs[g].a, alphal, st[b]->lqc, alphaq, a_idx[g], a_val[g]);
    scale[g] = alphal[cs[g].n - 1];
    for (size_t i = 0; i < nqt; ++i) u_quad[g * nqt + i] = ts[b].elt();
    pi[g] = a_idx[g].data();
    pv[g] = a_val[g].data();
    nsp[g] = a_idx[g].size();
    pdense[g] = d_eq + g * I.ninputs + st[b]->npub;
    lps[g] = lp[b];
  }
  std::vector<E> y_ldt(m * p.block), y_dot(m * p.dblock), y_q0(m * p.r + 1), y_q2(m * ymid + 1);
  LF_TRY(P::ligero_prove_batch(c, lps.data(), m, u_ldt.data(), pdense.data(), st[sel[0]]->n_witness, scale.data(), pi.data(), pv.data(), nsp.data(),
                               nqt ? u_quad.data() : nullptr, y_ldt.data(), y_dot.data(), y_q0.data(), y_q2.data()));
  std::vector<size_t> idx(m * p.nreq);
  for (size_t g = 0; g < m; ++g) {
    const size_t b = sel[g];
    ProofBody<E>& pr = st[b]->proof;
    pr.y_ldt.assign(y_ldt.begin() + g * p.block, y_ldt.begin() + (g + 1) * p.block);
    pr.y_dot.assign(y_dot.begin() + g * p.dblock, y_dot.begin() + (g + 1) * p.dblock);
    pr.y_q0.assign(y_q0.begin() + g * p.r, y_q0.begin() + (g + 1) * p.r);
    pr.y_q2.assign(y_q2.begin() + g * ymid, y_q2.begin() + (g + 1) * ymid);
    ts[b].write_array(pr.y_ldt.data(), pr.y_ldt.size());
    ts[b].write_array(pr.y_dot.data(), pr.y_dot.size());
    ts[b].write_array(pr.y_q0.data(), pr.y_q0.size());
    ts[b].write_array(pr.y_q2.data(), pr.y_q2.size());
    ts[b].choose(p.block_ext, p.nreq, idx.data() + g * p.nreq);
  }
  const size_t cap = p.nreq * p.mc_pathlen + 1;
  std::vector<E> req(m * p.nrow * p.nreq);
  std::vector<uint8_t> nonces(m * p.nreq * 32), path(m * cap * 32);
  std::vector<size_t> npath(m, 0);
  LF_TRY(P::ligero_open_batch(c, lps.data(), m, idx.data(), req.data(), nonces.data(), path.data(), cap, npath.data()));
  for (size_t g = 0; g < m; ++g) {
    ProofBody<E>& pr = st[sel[g]]->proof;
    pr.req.assign(req.begin() + g * p.nrow * p.nreq, req.begin() + (g + 1) * p.nrow * p.nreq);
    pr.nonces.assign(nonces.begin() + g * p.nreq * 32, nonces.begin() + (g + 1) * p.nreq * 32);
    pr.path.assign(cap * 32, 0);
    memcpy(pr.path.data(), path.data() + g * cap * 32, npath[g] * 32);
    pr.npath = npath[g];
    st[sel[g]]->have_proof = true;
  }
  ms[1] = now_ms() - t0;
  return LFGPU_OK;
}

// prove for statements 0 .. nb-1: pol[b], st[b], lp[b], h_W[b], tso[b] are statement b's; ok[b] as prove's *ok.  A statement
// whose witness fails rides along in the sumcheck on its transcript copy -- the launches are the batch's, not its own -- and
// what it produces is dropped: it holds no proof and its transcript is where the single call leaves it.
template <class P, class EqTable>
int prove_batch(lfgpu_ctx* c, const lfgpu_circuit* C, const P* pol, ProverState<P>* const* st, typename P::Lig* const* lp, const BatchBufs& bb, size_t nb,
                EqTable eq_table, const void* const* h_W, const lfgpu_transcript_ops* const* tso, int* ok) {
  using E = typename P::E;
  constexpr size_t B = P::kBytes;
  const double t_start = now_ms();
  const typename P::Field F = pol[0].host_field(c);
  const lfgpu_circuit_info& I = C->info;
  const size_t nl = C->layers.size();
  for (size_t b = 0; b < nb; ++b) {
    ok[b] = 0;
    st[b]->have_proof = false;
    st[b]->wire_valid = false;
  }
  LF_HIP(c, hipSetDevice(c->device));

  // eval_circuit of all statements: nl launches; the host hashes the nb preambles and clones the transcripts meanwhile
  double t0 = now_ms();
  for (size_t b = 0; b < nb; ++b)
    LF_HIP(c, hipMemcpyAsync((uint8_t*)bb.d_in[nl - 1] + b * bb.ldw[nl - 1] * B, h_W[b], I.ninputs * B, hipMemcpyHostToDevice, c->stream));
  LF_HIP(c, hipMemsetAsync(bb.d_fail, 0, nb * sizeof(int), c->stream));
  for (size_t l = nl; l-- > 0;)
    LF_TRY(P::eval_layer_batch(C->layers[l].q, nb, bb.d_in[l], bb.ldw[l], l ? bb.d_in[l - 1] : bb.d_V, l ? bb.ldw[l - 1] : bb.ldv, bb.d_fail));
  int* const h_fail = (int*)((uint8_t*)bb.h_V + bb.nb_max * bb.ldv * B);
  LF_HIP(c, hipMemcpyAsync(bb.h_V, bb.d_V, nb * bb.ldv * B, hipMemcpyDeviceToHost, c->stream));
  LF_HIP(c, hipMemcpyAsync(h_fail, bb.d_fail, nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  const double t_enq = now_ms() - t0;

  std::vector<Ts<P>> ts, tst;
  std::vector<CloneGuard> cg(nb, CloneGuard{nullptr, nullptr});
  ts.reserve(nb);
  tst.reserve(nb);
  for (size_t b = 0; b < nb; ++b) {
    ts.push_back(Ts<P>{&pol[b], tso[b], tso[b]->user});
    fs_init(ts[b], C, (const E*)h_W[b]);
    void* cl = tso[b]->clone(tso[b]->user);
    if (!cl) {
      (void)hipStreamSynchronize(c->stream);
      return lf_fail(c, LFGPU_ERR_NOMEM, "%s: transcript clone", P::kProveBatchName);
    }
    cg[b].o = tso[b];
    cg[b].u = cl;
    tst.push_back(Ts<P>{&pol[b], tso[b], cl});
  }

  t0 = now_ms();
  LF_HIP(c, hipStreamSynchronize(c->stream));
  std::vector<char> good(nb, 0);
  size_t ngood = 0;
  for (size_t b = 0; b < nb; ++b) {
    good[b] = witness_ok<P>((const E*)bb.h_V + b * bb.ldv, I.nv, h_fail[b]);
    ngood += good[b] ? 1 : 0;
  }
  const double ms_eval = t_enq + now_ms() - t0;
  if (!ngood) return LFGPU_OK;

  // padded sumcheck: one batched call per layer; G, alpha, beta, WC and aux are per statement
  t0 = now_ms();
  std::vector<ScRun<P>> run(nb);
  for (size_t b = 0; b < nb; ++b) sc_begin<P>(tst[b], C, *st[b], run[b]);
  std::vector<E> G0, G1, alpha(nb), beta(nb), wc_in(2 * nb), wc_out(2 * nb), bq(nb), gout;
  std::vector<RoundCtx<P>> rc;
  for (size_t ly = 0; ly < nl; ++ly) {
    const auto& L = C->layers[ly];
    const size_t logv = run[0].logv;
    G0.assign(nb * logv + 1, P::zero());
    G1.assign(nb * logv + 1, P::zero());
    rc.clear();
    for (size_t b = 0; b < nb; ++b) {
      rc.push_back(sc_layer_open<P>(F, tst[b], *st[b], ly, L.logw, &alpha[b], &beta[b]));
      for (size_t l = 0; l < logv; ++l) {
        G0[b * logv + l] = run[b].G[0][l];
        G1[b * logv + l] = run[b].G[1][l];
      }
      wc_in[2 * b] = run[b].WC[0];
      wc_in[2 * b + 1] = run[b].WC[1];
    }
    gout.assign(nb * 2 * L.logw + 1, P::zero());
    LF_TRY(P::sumcheck_layer_batch(L.q, F, nb, logv, G0.data(), G1.data(), alpha.data(), beta.data(), L.logw, L.nw, bb.d_in[ly], bb.ldw[ly], wc_in.data(),
                                   round_batch_cb<P>, rc.data(), wc_out.data(), gout.data(), bq.data()));
    for (size_t b = 0; b < nb; ++b) sc_layer_close<P>(F, tst[b], *st[b], ly, L.logw, &wc_out[2 * b], bq[b], &gout[b * 2 * L.logw], run[b]);
  }
  const double ms_sc = now_ms() - t0;

  // constraints, Ligero prove and open of the statements with a good witness: in three chains for all of them
  // (prove_finish_batch), or with the policy's switch at 0 (P::ligero_batch_switch: LFGPU_LIGERO_PROVE_BATCH for the 16-byte
  // fields, LFGPU_LIGERO_PROVE_BATCH256 for Fp256Base, each read once per process; the A/B switch, the same bytes) per
  // statement, one after the other, with the caller's EQ table reused
  const int lig_batched = P::ligero_batch_switch();
  for (size_t b = 0; b < nb; ++b) {
    st[b]->ms[2] = ms_eval;
    st[b]->ms[3] = ms_sc;
  }
  // The sumcheck does not look at the Ligero parameters, so provers of one circuit with different rate, nreq or block_enc are a
  // valid batch; their tableaux have different shapes, which the batched tail cannot take: such a batch keeps the per-statement loop.
  std::vector<size_t> sel;
  for (size_t b = 0; b < nb; ++b)
    if (good[b]) sel.push_back(b);
  bool one_shape = true;
  for (size_t g = 1; g < sel.size(); ++g)
    if (memcmp(&st[sel[g]]->param, &st[sel[0]]->param, sizeof(lfgpu_ligero_param)) != 0) one_shape = false;
  if (lig_batched && one_shape) {
    double ms_fin[2] = {0, 0};
    LF_TRY(prove_finish_batch<P>(c, C, F, st, lp, bb, sel, h_W, ts, ms_fin));
    for (size_t b = 0; b < nb; ++b) {
      st[b]->ms[4] = ms_fin[0];
      st[b]->ms[5] = ms_fin[1];
      if (good[b]) ok[b] = 1;
    }
  } else {
    for (size_t b = 0; b < nb; ++b) {
      if (!good[b]) continue;
      LF_TRY(prove_finish<P>(c, C, pol[b], F, *st[b], lp[b], eq_table, (const E*)h_W[b], ts[b]));
      ok[b] = 1;
    }
  }
  const double ms_all = now_ms() - t_start;
  for (size_t b = 0; b < nb; ++b) st[b]->ms[1] = ms_all;
  return LFGPU_OK;
}

// ------------------------------------------------------------------ ZkVerifier::recv_commitment + verify
// over the wire bytes of ZkProof::write.  Device work: bind_gh_all of every layer (the bulk: one pass over all corners of the
// circuit), the Reed-Solomon extension of the nwqrow rows of A and of the three y vectors, the gather at the opened columns
// (P::verifier_ext).  Host: transcript replay, symbolic constraints, the nreq column hashes and the Merkle recomputation.
// eq_table(E** d_eq): room for the EQ table over the inputs, asked for once the proof has parsed.
template <class P, class EqTable>
int verify(lfgpu_ctx* c, const lfgpu_circuit* C, const P& pol, const lfgpu_ligero_param& p, const uint8_t* proof, size_t proof_len, const void* h_pub,
           const lfgpu_transcript_ops* tso, bool committed, EqTable eq_table, int* ok, const char** why_out) {
  using E = typename P::E;
  const typename P::Field F = pol.host_field(c);
  auto fail = [&](int w) {
    if (why_out) *why_out = why_string(w);
    return LFGPU_OK;
  };
  const lfgpu_circuit_info& I = C->info;
  const size_t npub = I.npub_in, n_witness = I.ninputs - npub;
  static const bool verbose = getenv("LFGPU_VERBOSE") != nullptr;
  double tv[6] = {now_ms(), 0, 0, 0, 0, 0};
  ProofBody<E> pr;
  if (!proof_read(pol, C, p, proof, proof_len, pr)) return fail(kWhyParse);
  tv[1] = now_ms();
  LF_HIP(c, hipSetDevice(c->device));
  const Ts<P> ts{&pol, tso, tso->user};
  const E* pub = (const E*)h_pub;

  // recv_commitment (unless the caller has done it: ZkVerifier::recv_commitment and verify are separate calls, and the mdoc
  // verifier draws its MAC key between them, mdoc_zk.cc:676-681), initialize_sumcheck_fiat_shamir
  if (!committed) ts.write_bytes(pr.root, 32);
  fs_init(ts, C, pub);

  // verifier_constraints with aux == nullptr: the bound quad of every layer comes from bind_gh_all
  E* d_eq = nullptr;
  LF_TRY(eq_table(&d_eq));
  ConstraintSet<E> cs;
  LF_TRY(build_constraints<P>(c, C, F, ts, pr.sc, nullptr, pub, d_eq, cs));
  std::vector<size_t> lqc;
  pad_layout<P>(F, C, n_witness, lqc, [] { return P::zero(); }, nullptr, nullptr);
  tv[2] = now_ms();
  // LigeroVerifier::verify; A = the dense private-input block (the EQ table, on the device) + the sparse terms
  const uint8_t hash_of_A[32] = {0xde, 0xad, 0xbe, 0xef};
  auto ext_fn = [&](const std::vector<E>& alphal, const std::vector<E>& alphaq, const size_t* idx, std::vector<E>& ext) {
    std::vector<uint64_t> a_idx;
    std::vector<E> a_val;
    inner_product_sparse<P>(F, p, cs.a, alphal, lqc, alphaq, a_idx, a_val);
    return P::verifier_ext(c, F, I, p, d_eq, alphal[cs.n - 1], a_idx, a_val, pr, idx, ext);
  };
  int w = kWhyOk;
  LF_TRY(ligero_verify<P>(pol, F, p, pr.root, pr, ts, hash_of_A, cs.n, cs.b.data(), ext_fn, &w, tv));
  if (w != kWhyOk) return fail(w);
  if (verbose)
    fprintf(stderr, "lfgpu zk_verify: parse %.2f ms | FS init + constraints (bind_gh_all) %.2f | challenges + merkle %.2f | A + RS extension %.2f | checks %.2f\n",
            tv[1] - tv[0], tv[2] - tv[1], tv[3] - tv[2], tv[4] - tv[3], now_ms() - tv[4]);
  *ok = 1;
  return fail(kWhyOk);
}
}  // namespace
}  // namespace zkp
