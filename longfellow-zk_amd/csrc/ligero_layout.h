// ligero_layout.h -- the host half of LigeroProver::commit, written once over a host policy H.
//
// Reference: LigeroProver::commit / layout_blinding_rows / layout_witness_rows / layout_quadratic_rows
// (lib/ligero/ligero_prover.h:58-79,171-270), MerkleCommitment::commit's nonces (lib/merkle/merkle_commitment.h:52-54),
// RandomEngine::elt / subfield_elt (lib/random/random.h:38-48).
//
// Host only: no HIP runtime call and no lfgpu_ctx, so it also compiles into a --cuda-host-only harness
// (tests/host_ligero_layout.hip).  A host policy follows the Wire16 / Wire32 pattern of zk_proto.h: Host16 serves GF(2^128) and
// Fp128 and carries the field, Host32 serves Fp256Base.  It supplies E, field (the id), zero / is_zero / eq, add / sub / mul,
// sample / sample_subfield (n consecutive RandomEngine draws; how a width batches them into calls of the hook is its own
// business, and with `exact` every attempt, subfield element and nonce is one call of the reference's size) and
// first_outside_subfield, the witness check that opens the commit.  The width policies of ligero_slab.h derive from these.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "fp256.h"

// Everything below has internal linkage (as in zk_proto.h): each file that includes this header wants its own copy.
namespace lig {
namespace {
struct Host16 {
  using E = elt_t;
  int field, k;
  const GfHostCtx* g;  // GF(2^128): the subfield basis and its byte tables; the prime field needs none
  static E zero() { return elt_t{0, 0}; }
  static bool is_zero(E a) { return (a.lo | a.hi) == 0; }
  static bool eq(E a, E b) { return elt_eq(a, b); }
  E add(E a, E b) const { return field == LFGPU_FIELD_GF2_128 ? gf_add(a, b) : fp_add(a, b); }
  E sub(E a, E b) const { return field == LFGPU_FIELD_GF2_128 ? gf_add(a, b) : fp_sub(a, b); }
  E mul(E a, E b) const { return field == LFGPU_FIELD_GF2_128 ? gf_mul(a, b) : fp_mul(a, b); }
  // GF2_128::sample consumes exactly 16 bytes per element (gf2_128.h:182-190; little-endian host: the bytes are the Elt image),
  // so n draws of 16 bytes equal one draw of 16n bytes for every byte-stream RandomEngine of the reference (LCG test engines,
  // Transcript/FSPRF, SecureRandomEngine).  FpGeneric::sample (fp_generic.h:360-371) rejects >= p: element by element.
  void sample(E* out, size_t n, lfgpu_rng_fn rng, void* user, bool exact) const {
    if (field == LFGPU_FIELD_GF2_128 && !exact) return rng(user, reinterpret_cast<uint8_t*>(out), 16 * n);
    for (size_t i = 0; i < n; ++i) {
      do rng(user, reinterpret_cast<uint8_t*>(&out[i]), 16);
      while (field != LFGPU_FIELD_GF2_128 && !h_fp_fits(out[i]));
      if (field != LFGPU_FIELD_GF2_128) out[i] = h_fp_to_mont(out[i]);
    }
  }
  // GF2_128::sample_subfield (gf2_128.h:192-214): kSubFieldBytes little-endian bytes -> of_scalar, through the byte tables (the
  // mdoc hash circuit draws 34 000 of them per commit: 2.0 -> 0.2 ms of host time); FpGeneric::sample_subfield = sample
  void sample_subfield(E* out, size_t n, lfgpu_rng_fn rng, void* user, bool exact) const {
    if (field != LFGPU_FIELD_GF2_128) return sample(out, n, rng, user, exact);
    const size_t nb = g->sub_bits / 8;
    uint8_t buf[1024];
    for (size_t done = 0, m; done < n; done += m) {
      m = exact ? 1 : std::min(n - done, sizeof(buf) / nb);
      rng(user, buf, m * nb);
      for (size_t i = 0; i < m; ++i) {
        E t = g->sub_tab[0][buf[i * nb]];
        for (size_t b = 1; b < nb; ++b) t = gf_add(t, g->sub_tab[b][buf[i * nb + b]]);
        out[done + i] = t;
      }
    }
  }
  // GF2_128::in_subfield (gf2_128.h:201-204) over W[0, n): the index of the first element outside the subfield, or n.  beta in
  // echelon form; an element lies in the subfield iff cancelling its pivot bits leaves nothing.  Identically true for Fp128.
  size_t first_outside_subfield(const E* W, size_t n) const {
    if (field != LFGPU_FIELD_GF2_128 || n == 0) return n;
    auto top_bit = [](E e) { return e.hi ? 64 + (63 - __builtin_clzll(e.hi)) : 63 - __builtin_clzll(e.lo); };
    auto bit_of = [](E e, int j) { return j >= 64 ? (e.hi >> (j - 64)) & 1 : (e.lo >> j) & 1; };
    E v[32];
    int pivot[32];
    unsigned nv = 0;
    auto reduce = [&](E e) {  // a row's pivot bit is clear in every LATER row: one pass in order
      for (unsigned r = 0; r < nv; ++r)
        if (bit_of(e, pivot[r])) e = gf_add(e, v[r]);
      return e;
    };
    for (unsigned i = 0; i < g->sub_bits && i < 32; ++i) {
      v[nv] = reduce(g->beta[i]);  // beta is a basis: never zero
      pivot[nv] = top_bit(v[nv]);
      ++nv;
    }
    for (size_t i = 0; i < n; ++i)
      if ((W[i].hi || W[i].lo > 1) && !is_zero(reduce(W[i]))) return i;  // 0 and 1: nearly every input of a bit circuit
    return n;
  }
};

struct Host32 {  // Fp256Base: FpGeneric::sample and sample_subfield are the same function (fp_generic.h:360-376)
  using E = elt32_t;
  static constexpr int field = LFGPU_FIELD_P256;
  static E zero() { return e32_zero(); }
  static bool is_zero(const E& a) { return e32_is_zero(a); }
  static bool eq(const E& a, const E& b) { return e32_eq(a, b); }
  static E add(const E& a, const E& b) { return fp256_add(a, b); }
  static E sub(const E& a, const E& b) { return fp256_sub(a, b); }
  static E mul(const E& a, const E& b) { return fp256_mul(a, b); }
  // 32 bytes per attempt: the bulk rejection loop of h256_sample_many (fp256.h), or one call per attempt
  static void sample(E* out, size_t n, lfgpu_rng_fn rng, void* user, bool exact) {
    auto fill = [&](uint8_t* b, size_t nb) { rng(user, b, nb); };
    if (!exact) return h256_sample_many(out, n, fill);
    for (size_t i = 0; i < n; ++i) out[i] = h256_sample(fill);
  }
  static void sample_subfield(E* out, size_t n, lfgpu_rng_fn rng, void* user, bool exact) { sample(out, n, rng, user, exact); }
  static size_t first_outside_subfield(const E*, size_t n) { return n; }
};

// Every RandomEngine draw of the commit in the reference's order (they do not depend on computed data); the un-encoded image
// (first dblock columns) of rows [row_lo, row_hi) goes to Himg ([row_hi - row_lo][dblock]).  Rows outside the slab are drawn
// into a spare row and dropped, so that ranks which replay the same byte stream hold consistent slabs of ONE tableau; the empty
// slab [0, 0) only advances the engine.  nonces (block_ext * 32 bytes) may be null: the draw still happens.  Returns LFGPU_OK /
// LFGPU_ERR_ARG / LFGPU_ERR_ASSERT with a message in err (256 bytes).
template <class H>
int layout(const H& hp, const lfgpu_ligero_param& p, const typename H::E* W, size_t subfield_boundary, const size_t* lqc, lfgpu_rng_fn rng, void* user,
           bool exact, size_t row_lo, size_t row_hi, typename H::E* Himg, uint8_t* nonces, char* err) {
  using E = typename H::E;
  // the check that opens LigeroProver::commit (ligero_prover.h:63-66), before any draw: a row below the boundary is blinded
  // with subfield randomness, which hides nothing of a full-field value in it
  const size_t nsub = std::min(subfield_boundary, p.nw), bad = hp.first_outside_subfield(W, nsub);
  if (bad < nsub) {
    snprintf(err, 256, "ligero_commit: element not in subfield: W[%zu], below subfield_boundary %zu (ligero_prover.h:63-66)", bad, subfield_boundary);
    return LFGPU_ERR_ARG;
  }
  const size_t hw = p.dblock;
  std::vector<E> spare(hw);
  LF_SCRUB_ON_EXIT(spare);
  auto own = [&](size_t i) { return i >= row_lo && i < row_hi; };
  auto row = [&](size_t i) { return own(i) ? Himg + (i - row_lo) * hw : spare.data(); };
  if (row_hi > row_lo) std::fill(Himg, Himg + (row_hi - row_lo) * hw, hp.zero());
  // layout_blinding_rows (:171-205)
  hp.sample(row(p.ildt), p.block, rng, user, exact);
  {
    E* d = row(p.idot);
    hp.sample(d, p.dblock, rng, user, exact);
    E sum = hp.zero();
    for (size_t j = 0; j < p.w; ++j) sum = hp.add(sum, d[p.r + j]);
    d[p.r] = hp.sub(d[p.r], sum);
  }
  {
    E* q = row(p.iquad);
    hp.sample(q, p.dblock, rng, user, exact);
    for (size_t j = 0; j < p.w; ++j) q[p.r + j] = hp.zero();
  }
  // layout_witness_rows (:207-231)
  for (size_t i = 0; i < p.nwrow; ++i) {
    E* t = row(i + p.iw);
    if ((i + 1) * p.w <= subfield_boundary) hp.sample_subfield(t, p.r, rng, user, exact);
    else hp.sample(t, p.r, rng, user, exact);
    if (!own(i + p.iw)) continue;
    const size_t max_col = std::min(p.w, p.nw - i * p.w);
    for (size_t j = 0; j < max_col; ++j) t[p.r + j] = W[i * p.w + j];
  }
  // layout_quadratic_rows (:233-270)
  const size_t iqx = p.iq, iqy = iqx + p.nqtriples, iqz = iqy + p.nqtriples;
  for (size_t i = 0; i < p.nqtriples; ++i) {
    hp.sample(row(iqx + i), p.r, rng, user, exact);
    hp.sample(row(iqy + i), p.r, rng, user, exact);
    hp.sample(row(iqz + i), p.r, rng, user, exact);
    for (size_t j = 0; j < p.w && j + i * p.w < p.nq; ++j) {
      const size_t* l = &lqc[3 * (j + i * p.w)];
      if (l[0] >= p.nw || l[1] >= p.nw || l[2] >= p.nw) {
        snprintf(err, 256, "ligero_commit: lqc index >= nw");
        return LFGPU_ERR_ARG;
      }
      if (!hp.eq(hp.mul(W[l[0]], W[l[1]]), W[l[2]])) {
        snprintf(err, 256, "ligero_commit: invalid quadratic constraints (ligero_prover.h:259-260)");
        return LFGPU_ERR_ASSERT;
      }
      if (own(iqx + i)) row(iqx + i)[j + p.r] = W[l[0]];
      if (own(iqy + i)) row(iqy + i)[j + p.r] = W[l[1]];
      if (own(iqz + i)) row(iqz + i)[j + p.r] = W[l[2]];
    }
  }
  // MerkleCommitment::commit draws one 32-byte nonce per leaf, after the layout (merkle_commitment.h:52-54): one draw of
  // 32 * block_ext bytes is the same stream for every byte-stream engine
  std::vector<uint8_t> drop(nonces ? 0 : 32 * p.block_ext);
  if (!nonces) nonces = drop.data();
  if (!exact) rng(user, nonces, 32 * p.block_ext);
  else for (size_t j = 0; j < p.block_ext; ++j) rng(user, nonces + 32 * j, 32);
  return LFGPU_OK;
}
}  // namespace
}  // namespace lig
