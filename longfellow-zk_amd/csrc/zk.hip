// zk.hip -- host driver of the ZK prover over the device kernels (include/lfgpu_zk.h).
//
// Host control flow restated from the reference (no reference code is linked or copied):
//   Transcript / FSPRF                 lib/random/transcript.h:33-190, lib/random/random.h:57-105
//   CircuitRep::from_bytes (LFC1)      lib/proto/circuit_reader.h:55-233, circuit_writer.h:103-114
//   ZkProver::commit / fill_pad        lib/zk/zk_prover.h:72-96,152-188
//   ZkProver::prove                    lib/zk/zk_prover.h:98-149
//   ProverLayers::prove (padded)       lib/sumcheck/prover_layers.h:106-183,320-344
//   ZkCommon::verifier_constraints     lib/zk/zk_common.h:49-136,406-439
//   LigeroProver::prove                lib/ligero/ligero_prover.h:84-146, inner_product_vector ligero_param.h:382-421
//   ZkProof::write                     lib/zk/zk_proof.h:90-185
// Every data-parallel step is a kernel behind lfgpu.h (eval_quad, sumcheck_layer, raw_eq2, ligero_*); what runs
// on the host is the sequential bookkeeping the reference also keeps there.  The protocol layer itself (transcript view,
// fill_pad, prove, verifier_constraints, ZkProof::write / read, verify) is zk_proto.h, shared with zk256.hip: this file holds
// the transcript object, the LFC1 reader, the 16-byte policy with its device adapters, commit and the C entry points.
// This file has no device code.
#include <algorithm>
#include <memory>

#include "zk_driver.h"

extern "C" int lfgpu_raw_eq2(lfgpu_ctx*, int, size_t, size_t, const void*, const void*, const uint64_t*, void*);

using zkp::elt_of_bytes;
using zkp::kMaxBindings;
using zkp::layer_size;
using zkp::now_ms;

// ------------------------------------------------------------------ built-in transcript
struct lfgpu_transcript {  // Transcript + FSPRF (lib/random/transcript.h:33-190)
  Sha256 sha;
  bool prf = false;
  Aes256 aes;
  u64 nblock = 0;
  uint8_t saved[16];
  size_t rdptr = 16;
  void upd(const uint8_t* p, size_t n) {
    prf = false;  // any write invalidates the PRF (:174-178)
    sha.update(p, n);
  }
  void tag_len(uint8_t tag, u64 n) {
    uint8_t h[9] = {tag};
    for (int i = 0; i < 8; ++i) h[1 + i] = (uint8_t)(n >> (8 * i));
    upd(h, 9);
  }
  void write_bytes(const uint8_t* d, size_t n) {  // tag 0 || u64 length || bytes (:115-120)
    tag_len(0, n);
    if (n) upd(d, n);
  }
  void write_elt(const uint8_t* e, size_t nbytes = 16) {  // tag 1 || image (:136-140)
    const uint8_t t = 1;
    upd(&t, 1);
    upd(e, nbytes);
  }
  void write_elt_array(const uint8_t* e, size_t n, size_t nbytes = 16) {  // tag 2 || u64 count || images (:144-152)
    tag_len(2, n);
    if (n) upd(e, nbytes * n);
  }
  void bytes(uint8_t* out, size_t n) {
    if (!prf) {  // key = SHA-256 of a copy of the running state (:160-172)
      uint8_t key[32];
      sha.digest(key);
      aes.set_key(key);
      nblock = 0;
      rdptr = 16;
      prf = true;
    }
    while (n) {
      if (rdptr == 16) {
        if (n >= 16) {  // whole blocks straight into the output (bulk RandomEngine draws)
          const size_t nb = n / 16;
          aes.ctr_blocks(nblock, nb, out);
          nblock += nb;
          out += 16 * nb;
          n -= 16 * nb;
          continue;
        }
        aes.ctr_blocks(nblock, 1, saved);  // FSPRF::refill (:53-60): AES(LE64 counter || 0^8)
        ++nblock;
        rdptr = 0;
      }
      const size_t take = n < 16 - rdptr ? n : 16 - rdptr;
      memcpy(out, saved + rdptr, take);
      out += take; rdptr += take; n -= take;
    }
  }
};

extern "C" {
lfgpu_transcript* lfgpu_transcript_new(const uint8_t* init, size_t n) {
  if (n && !init) return nullptr;
  lfgpu_transcript* t = new (std::nothrow) lfgpu_transcript();
  if (t) t->write_bytes(init, n);
  return t;
}
void lfgpu_transcript_free(lfgpu_transcript* t) { delete t; }
void lfgpu_transcript_write_bytes(lfgpu_transcript* t, const uint8_t* d, size_t n) { t->write_bytes(d, n); }
void lfgpu_transcript_write_elt(lfgpu_transcript* t, const uint8_t* e) { t->write_elt(e); }
void lfgpu_transcript_write_elt_array(lfgpu_transcript* t, const uint8_t* e, size_t n) { t->write_elt_array(e, n); }
void lfgpu_transcript_bytes(lfgpu_transcript* t, uint8_t* out, size_t n) { t->bytes(out, n); }
void lfgpu_transcript_write_elt_sized(lfgpu_transcript* t, const uint8_t* e, size_t nbytes) { t->write_elt(e, nbytes); }
void lfgpu_transcript_write_elt_array_sized(lfgpu_transcript* t, const uint8_t* e, size_t n, size_t nbytes) { t->write_elt_array(e, n, nbytes); }
void lfgpu_sha256(const uint8_t* data, size_t n, uint8_t out[32]) {
  Sha256 s;
  s.update(data, n);
  s.digest(out);
}
void lfgpu_host_gf2128_mul(const uint64_t a[2], const uint64_t b[2], uint64_t out[2]) {
  const elt_t r = h_gf_mul(elt_t{a[0], a[1]}, elt_t{b[0], b[1]});
  out[0] = r.lo;
  out[1] = r.hi;
}
int lfgpu_crypto_hw(int force_portable) {
  if (force_portable >= 0) fs_crypto_force_portable(force_portable);
  return fs_crypto_hw();
}
void lfgpu_aes256_ecb_block(const uint8_t key[32], const uint8_t in[16], uint8_t out[16]) {
  Aes256 a;
  a.set_key(key);
  a.encrypt(in, out);
}
static void op_write_bytes(void* u, const uint8_t* d, size_t n) { ((lfgpu_transcript*)u)->write_bytes(d, n); }
static void op_write_elt(void* u, const uint8_t* e) { ((lfgpu_transcript*)u)->write_elt(e); }
static void op_write_arr(void* u, const uint8_t* e, size_t n) { ((lfgpu_transcript*)u)->write_elt_array(e, n); }
static void op_bytes(void* u, uint8_t* o, size_t n) { ((lfgpu_transcript*)u)->bytes(o, n); }
static void op_write_elt_sized(void* u, const uint8_t* e, size_t nb) { ((lfgpu_transcript*)u)->write_elt(e, nb); }
static void op_write_arr_sized(void* u, const uint8_t* e, size_t n, size_t nb) { ((lfgpu_transcript*)u)->write_elt_array(e, n, nb); }
static void* op_clone(void* u) {  // Transcript::clone copies the hash state only; the PRF restarts (:95-99)
  lfgpu_transcript* t = new (std::nothrow) lfgpu_transcript();
  if (t) t->sha = ((lfgpu_transcript*)u)->sha;
  return t;
}
static void op_free(void* u) { delete (lfgpu_transcript*)u; }
void lfgpu_transcript_get_ops(lfgpu_transcript* t, lfgpu_transcript_ops* ops) {
  ops->user = t;
  ops->write_bytes = op_write_bytes;
  ops->write_elt = op_write_elt;
  ops->write_elt_array = op_write_arr;
  ops->gen_bytes = op_bytes;
  ops->clone = op_clone;
  ops->free_clone = op_free;
  ops->write_elt_sized = op_write_elt_sized;
  ops->write_elt_array_sized = op_write_arr_sized;
}
}  // extern "C"

// ------------------------------------------------------------------ circuit
extern "C" int lfgpu_circuit_from_lfc1(lfgpu_ctx* c, const uint8_t* b, size_t len, lfgpu_circuit** out) {
  if (!c || !b || !out) return LFGPU_ERR_ARG;
  size_t pos = 0;
  auto need = [&](size_t n) { return len - pos >= n; };
  auto num = [&](size_t* v) {  // 3-byte little-endian (circuit_reader.h:217-233)
    if (!need(3)) return false;
    *v = (size_t)b[pos] | (size_t)b[pos + 1] << 8 | (size_t)b[pos + 2] << 16;
    pos += 3;
    return true;
  };
  if (len < 1 || b[0] != 1) return lf_fail(c, LFGPU_ERR_ARG, "LFC1: bad version byte");
  pos = 1;
  size_t fid, nv, nc, npub, sfb, nin, nl, nk;
  if (!num(&fid) || !num(&nv) || !num(&nc) || !num(&npub) || !num(&sfb) || !num(&nin) || !num(&nl) || !num(&nk))
    return lf_fail(c, LFGPU_ERR_ARG, "LFC1: truncated header");
  if (fid != LFGPU_FIELD_GF2_128 && fid != LFGPU_FIELD_FP128 && fid != LFGPU_FIELD_P256)
    return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "LFC1: field id %zu (the ZK driver handles GF2_128 = 4, Fp128 = 6 and Fp256Base = 1)", fid);
  const int field = (int)fid;
  const size_t esz = field == LFGPU_FIELD_P256 ? 32 : 16;  // Field::kBytes
  if (nc != 1) return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "LFC1: nc = %zu copies (logc must be 0)", nc);
  // CircuitReader::read_header's sanity checks (lib/proto/circuit_reader.h:104-110): an oversized subfield_boundary would
  // mark every witness row subfield-only, including the rows that hold the full-field sumcheck pads
  if (npub > nin || sfb > nin || nv == 0 || nl == 0 || nl > 10000 /* CircuitIO::kMaxLayers */) return lf_fail(c, LFGPU_ERR_ARG, "LFC1: inconsistent header");
  if (nk > (len - pos) / esz) return lf_fail(c, LFGPU_ERR_ARG, "LFC1: truncated constant table");
  std::vector<elt_t> kvec((nk ? nk : 1) * (esz / 16));  // Fp256Base: nk 32-byte elements in the same storage
  for (size_t i = 0; i < nk; ++i) {  // of_bytes_field: kBytes little-endian bytes (prime fields: canonical value -> Montgomery)
    const bool fits = field == LFGPU_FIELD_P256 ? h256_of_bytes(b + pos + 32 * i, reinterpret_cast<elt32_t*>(kvec.data())[i])
                                                : elt_of_bytes(field, b + pos + 16 * i, kvec[i]);
    if (!fits) return lf_fail(c, LFGPU_ERR_ARG, "LFC1: constant %zu is not a field element", i);
  }
  pos += esz * nk;
  std::unique_ptr<lfgpu_circuit> C(new lfgpu_circuit());
  C->c = c;
  size_t nterms = 0, nout = nv;
  std::vector<corner4> corners;
  const double t_begin = now_ms();
  double t_upload = 0;
  for (size_t ly = 0; ly < nl; ++ly) {
    size_t logw, nw, nq;
    if (!num(&logw) || !num(&nw) || !num(&nq)) return lf_fail(c, LFGPU_ERR_ARG, "LFC1: truncated layer header");
    // read_layers (circuit_reader.h:161-168): lw in (0, kMaxBindings], 0 < nw, lw <= nw <= 2^lw, nq > 0
    if (logw > kMaxBindings || logw == 0 || nw == 0 || nw < logw || nw > ((size_t)1 << logw) || nq == 0 || !need(12 * nq))
      return lf_fail(c, LFGPU_ERR_ARG, "LFC1: bad layer %zu", ly);
    corners.resize(nq);
    int64_t acc[3] = {0, 0, 0};
    const uint8_t* q = b + pos;  // 12 * nq bytes are there (checked above): four 3-byte little-endian numbers per term
    size_t hmax = 0;
    for (size_t t = 0; t < nq; ++t, q += 12) {
      u32 v[4];
      for (int j = 0; j < 4; ++j) v[j] = (u32)q[3 * j] | (u32)q[3 * j + 1] << 8 | (u32)q[3 * j + 2] << 16;
      for (int j = 0; j < 3; ++j) {  // delta with the sign in the LSB (circuit_writer.h:103-114)
        const int64_t d = (int64_t)(v[j] >> 1);
        acc[j] += (v[j] & 1) ? -d : d;
      }
      if (acc[0] < 0 || (size_t)acc[0] >= nout || acc[1] < 0 || (size_t)acc[1] >= nw || acc[2] < 0 || (size_t)acc[2] >= nw || v[3] >= nk)
        return lf_fail(c, LFGPU_ERR_ARG, "LFC1: layer %zu term %zu out of range", ly, t);
      corners[t] = corner4{(u32)acc[0], (u32)acc[1], (u32)acc[2], v[3]};
      hmax = std::max<size_t>(hmax, (size_t)std::max(acc[1], acc[2]));
    }
    pos += 12 * nq;
    lfgpu_circuit::Layer L{logw, nw, nq, nullptr};
    const double tu0 = now_ms();
    LF_TRY(lf_quad_upload_corners(c, field, nq, corners.data(), hmax, nk, kvec.data(), nout, &L.q));  // indices range-checked above
    t_upload += now_ms() - tu0;
    C->layers.push_back(L);
    nterms += nq;
    nout = nw;
  }
  if (!need(32) || pos + 32 != len) return lf_fail(c, LFGPU_ERR_ARG, "LFC1: bad trailer");
  if (nout != nin) return lf_fail(c, LFGPU_ERR_ARG, "LFC1: input layer width %zu != ninputs %zu", nout, nin);
  if (getenv("LFGPU_VERBOSE"))
    fprintf(stderr, "lfgpu circuit_from_lfc1: %zu terms in %zu layers: %.1f ms (decode %.1f, lfgpu_quad_upload %.1f)\n", nterms, nl, now_ms() - t_begin,
            now_ms() - t_begin - t_upload, t_upload);
  lfgpu_circuit_info& I = C->info;
  I.field = field;
  I.nv = nv; I.nc = nc; I.npub_in = npub; I.subfield_boundary = sfb; I.ninputs = nin; I.nl = nl; I.nterms = nterms;
  C->zeros = std::make_shared<const std::vector<uint8_t>>(nterms, (uint8_t)0);
  I.logv = lf_log2(nv);
  memcpy(I.id, b + pos, 32);
  *out = C.release();
  return LFGPU_OK;
}
// A second handle on an uploaded circuit for another context of the same device: the device arrays of every layer and the
// preamble's zero run are shared (reference-counted; either handle may be freed first), the per-proof caches are the handle's own.
extern "C" int lfgpu_circuit_share(lfgpu_ctx* c, const lfgpu_circuit* src, lfgpu_circuit** out) {
  if (!c || !src || !out) return LFGPU_ERR_ARG;
  if (c->device != src->c->device) return lf_fail(c, LFGPU_ERR_ARG, "circuit_share: the contexts are on different devices");
  LF_HIP(c, hipSetDevice(c->device));
  LF_HIP(c, hipStreamSynchronize(src->c->stream));  // the upload is complete (lfgpu_circuit_from_lfc1 synchronises; cheap)
  std::unique_ptr<lfgpu_circuit> C(new lfgpu_circuit());
  C->c = c;
  C->info = src->info;
  C->zeros = src->zeros;
  for (const auto& l : src->layers) {
    lfgpu_circuit::Layer L{l.logw, l.nw, l.nterms, nullptr};
    LF_TRY(lf_quad_share(c, l.q, &L.q));
    C->layers.push_back(L);
  }
  *out = C.release();
  return LFGPU_OK;
}
extern "C" int lfgpu_circuit_get_info(const lfgpu_circuit* C, lfgpu_circuit_info* info) {
  if (!C || !info) return LFGPU_ERR_ARG;
  *info = C->info;
  return LFGPU_OK;
}
extern "C" int lfgpu_circuit_layer_info(const lfgpu_circuit* C, size_t layer, size_t* logw, size_t* nw, size_t* nterms) {
  if (!C || layer >= C->layers.size()) return LFGPU_ERR_ARG;
  if (logw) *logw = C->layers[layer].logw;
  if (nw) *nw = C->layers[layer].nw;
  if (nterms) *nterms = C->layers[layer].nterms;
  return LFGPU_OK;
}
extern "C" int lfgpu_circuit_free(lfgpu_circuit* C) {
  if (!C) return LFGPU_ERR_ARG;
  delete C;
  return LFGPU_OK;
}

// ------------------------------------------------------------------ the 16-byte policy
namespace {
// The EQ table over the circuit inputs is context-owned and grown on demand: it stays valid until the next run on this context
int zk_eq_reserve(lfgpu_ctx* c, size_t ninputs) {
  if (c->zk_eq_bytes >= ninputs * 16) return LFGPU_OK;
  LF_HIP(c, hipSetDevice(c->device));
  LF_HIP(c, hipStreamSynchronize(c->stream));
  if (c->zk_eq) hipFree(c->zk_eq);
  c->zk_eq = nullptr;
  c->zk_eq_bytes = 0;
  if (hipMalloc(&c->zk_eq, ninputs * 16) != hipSuccess) return lf_fail(c, LFGPU_ERR_NOMEM, "zk: EQ table over the inputs");
  c->zk_eq_bytes = ninputs * 16;
  return LFGPU_OK;
}
// Wire16 (zk_proto.h) plus the device steps behind lfgpu.h.  elt_t is {lo, hi}: the scalars the C ABI takes as uint64_t[2]
// are copied here and nowhere else.
struct P16 : zkp::Wire16 {
  using Lig = lfgpu_ligero_prover;
  using Layer = lfgpu_circuit::Layer;
  typedef void (*round_fn)(void* user, size_t hand, size_t rnd, const E ev[3], E* chal);
  static constexpr const char* kProveName = "zk_prove";
  HostField host_field(lfgpu_ctx* c) const { return HostField(c, field); }
  // the verifier's bind_gh_all sums of up to LF_GH_BATCH_MAX layers wait in the device mailbox for one read-back
  static constexpr bool kDeferGh = true;
  static constexpr size_t kGhBatchMax = LF_GH_BATCH_MAX;
  struct W2 {
    uint64_t v[2];
    W2(const E& e) : v{e.lo, e.hi} {}
  };
  static int eval_layer(lfgpu_quad* q, const void* d_W, void* d_V, int* d_fail) { return lf_eval_quad_async(q, d_W, d_V, d_fail); }
  struct Tramp {
    round_fn f;
    void* user;
  };
  static void tramp_cb(void* user, size_t hand, size_t rnd, const uint64_t ev[3][2], uint64_t chal[2]) {
    const Tramp* t = (const Tramp*)user;
    const E e[3] = {E{ev[0][0], ev[0][1]}, E{ev[1][0], ev[1][1]}, E{ev[2][0], ev[2][1]}};
    E ch;
    t->f(t->user, hand, rnd, e, &ch);
    chal[0] = ch.lo;
    chal[1] = ch.hi;
  }
  static int sumcheck_layer(lfgpu_quad* q, const HostField&, size_t logv, const E* G0, const E* G1, const E& alpha, const E& beta, size_t logw, size_t nw,
                            void* d_W, const E wc_in[2], round_fn round, void* user, E wc_out[2], E* g_out /*[2][logw]*/, E* bound_quad) {
    Tramp t{round, user};
    const uint64_t WC[2][2] = {{wc_in[0].lo, wc_in[0].hi}, {wc_in[1].lo, wc_in[1].hi}};
    uint64_t wo[2][2], bq[2];
    std::vector<uint64_t> g(4 * logw + 2, 0);
    LF_TRY(lfgpu_sumcheck_layer(q, logv, G0, G1, W2(alpha).v, W2(beta).v, logw, nw, d_W, WC, tramp_cb, &t, wo, g.data(), bq));
    wc_out[0] = E{wo[0][0], wo[0][1]};
    wc_out[1] = E{wo[1][0], wo[1][1]};
    for (size_t i = 0; i < 2 * logw; ++i) g_out[i] = E{g[2 * i], g[2 * i + 1]};
    *bound_quad = E{bq[0], bq[1]};
    return LFGPU_OK;
  }
  // ---- the batch axis (zkp::prove_batch): B statements of one layer per call
  typedef void (*round_batch_fn)(void* user, size_t hand, size_t rnd, size_t nb, const E (*ev)[3], E* chal);
  static constexpr const char* kProveBatchName = "zk_prove_batch";
  // LFGPU_LIGERO_PROVE_BATCH [1] (read once per process): 0 = constraints, Ligero prove and opening per statement (prove_finish)
  static int ligero_batch_switch() {
    static const int on = getenv("LFGPU_LIGERO_PROVE_BATCH") ? atoi(getenv("LFGPU_LIGERO_PROVE_BATCH")) : 1;
    return on;
  }
  static int eval_layer_batch(lfgpu_quad* q, size_t nb, const void* d_W, size_t ldw, void* d_V, size_t ldv, int* d_fail) {
    return lf_eval_quad_batch_async(q, nb, d_W, ldw, d_V, ldv, d_fail);
  }
  struct TrampBatch {
    round_batch_fn f;
    void* user;
    std::vector<E> ev, ch;
  };
  static void tramp_batch_cb(void* user, size_t hand, size_t rnd, size_t nb, const uint64_t (*ev)[3][2], uint64_t (*chal)[2]) {
    TrampBatch* t = (TrampBatch*)user;
    for (size_t b = 0; b < nb; ++b)
      for (int k = 0; k < 3; ++k) t->ev[3 * b + k] = E{ev[b][k][0], ev[b][k][1]};
    t->f(t->user, hand, rnd, nb, (const E(*)[3])t->ev.data(), t->ch.data());
    for (size_t b = 0; b < nb; ++b) {
      chal[b][0] = t->ch[b].lo;
      chal[b][1] = t->ch[b].hi;
    }
  }
  // G0 / G1: [nb][logv]; alpha, beta, bound_quad: [nb]; wc_in, wc_out: [nb][2]; g_out: [nb][2][logw]; d_W: statement b at b * ldw
  static int sumcheck_layer_batch(lfgpu_quad* q, const HostField&, size_t nb, size_t logv, const E* G0, const E* G1, const E* alpha, const E* beta, size_t logw,
                                  size_t nw, void* d_W, size_t ldw, const E* wc_in, round_batch_fn round, void* user, E* wc_out, E* g_out, E* bound_quad) {
    TrampBatch t{round, user, std::vector<E>(3 * nb), std::vector<E>(nb)};
    std::vector<uint64_t> al(2 * nb), be(2 * nb), wi(4 * nb), wo(4 * nb), bq(2 * nb), g(4 * nb * logw + 2, 0);
    for (size_t b = 0; b < nb; ++b) {
      al[2 * b] = alpha[b].lo; al[2 * b + 1] = alpha[b].hi;
      be[2 * b] = beta[b].lo; be[2 * b + 1] = beta[b].hi;
      for (int k = 0; k < 2; ++k) {
        wi[4 * b + 2 * k] = wc_in[2 * b + k].lo;
        wi[4 * b + 2 * k + 1] = wc_in[2 * b + k].hi;
      }
    }
    LF_TRY(lfgpu_sumcheck_layer_batch(q, nb, logv, G0, G1, al.data(), be.data(), logw, nw, d_W, ldw, wi.data(), tramp_batch_cb, &t, wo.data(), g.data(), bq.data()));
    for (size_t b = 0; b < nb; ++b) {
      wc_out[2 * b] = E{wo[4 * b], wo[4 * b + 1]};
      wc_out[2 * b + 1] = E{wo[4 * b + 2], wo[4 * b + 3]};
      bound_quad[b] = E{bq[2 * b], bq[2 * b + 1]};
    }
    for (size_t i = 0; i < 2 * nb * logw; ++i) g_out[i] = E{g[2 * i], g[2 * i + 1]};
    return LFGPU_OK;
  }
  static int bind_gh_all(lfgpu_ctx*, const HostField&, const Layer& L, size_t logv, const E* G0, const E* G1, const E& alpha, const E& beta, const E* H0,
                         const E* H1, E* out) {
    uint64_t bq[2];
    LF_TRY(lfgpu_quad_bind_gh_all(L.q, logv, G0, G1, W2(alpha).v, W2(beta).v, L.logw, L.nw, H0, H1, bq));
    *out = E{bq[0], bq[1]};
    return LFGPU_OK;
  }
  static int gh_enqueue(lfgpu_ctx* c, const Layer& L, size_t logv, const E* G0, const E* G1, const E& alpha, const E& beta, const E* H0, const E* H1,
                        size_t slot) {
    return lf_quad_bind_gh_all_enqueue(L.q, logv, G0, G1, W2(alpha).v, W2(beta).v, L.logw, L.nw, H0, H1, (u64*)((uint8_t*)c->mailbox_d + 512) + 4 * slot);
  }
  static int gh_read(lfgpu_ctx* c, const HostField& F, size_t nl, std::vector<E>& out) {
    std::vector<u64> w(4 * nl);
    LF_HIP(c, hipMemcpyAsync(w.data(), (uint8_t*)c->mailbox_d + 512, nl * 32, hipMemcpyDeviceToHost, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));
    out.resize(nl);
    for (size_t i = 0; i < nl; ++i) {
      uint64_t bq[2];
      lf_quad_bind_gh_all_fold(F.field, &w[4 * i], bq);
      out[i] = E{bq[0], bq[1]};
    }
    return LFGPU_OK;
  }
  // EQ(H0, i) + alpha EQ(H1, i), i < n, into d_eq; its first npub entries back to the host
  static int eq_table(lfgpu_ctx* c, const HostField& F, size_t logn, size_t n, const E* H0, const E* H1, const E& alpha, E* d_eq, size_t npub, E* eq_in) {
    LF_TRY(lfgpu_raw_eq2(c, F.field, logn, n, H0, H1, W2(alpha).v, d_eq));
    if (npub) LF_HIP(c, hipMemcpyAsync(eq_in, d_eq, npub * 16, hipMemcpyDeviceToHost, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));
    return LFGPU_OK;
  }
  // ... for nb statements in one launch: H0 / H1 [nb][logn], statement b's table at d_eq + b * n, its first npub entries to
  // eq_in + b * npub in one read-back
  static int eq_table_batch(lfgpu_ctx* c, const HostField& F, size_t nb, size_t logn, size_t n, const E* H0, const E* H1, const E* alpha, E* d_eq,
                            size_t npub, E* eq_in) {
    std::vector<uint64_t> al(2 * nb);
    for (size_t b = 0; b < nb; ++b) {
      al[2 * b] = alpha[b].lo;
      al[2 * b + 1] = alpha[b].hi;
    }
    LF_TRY(lf_raw_eq2_batch(c, F.field, nb, logn, n, H0, H1, al.data(), d_eq));
    if (npub) {  // (without public inputs nothing is read: the tables are consumed in stream order by the dot proofs)
      LF_HIP(c, hipMemcpy2DAsync(eq_in, npub * 16, d_eq, n * 16, npub * 16, nb, hipMemcpyDeviceToHost, c->stream));
      LF_HIP(c, hipStreamSynchronize(c->stream));
    }
    return LFGPU_OK;
  }
  static int low_degree(Lig* lp, const E* u, E* y) { return lfgpu_ligero_low_degree_proof(lp, u, y); }
  static int dot(Lig* lp, const E* d_dense, size_t ndense, const E& scale, const uint64_t* idx, const E* val, size_t nsparse, E* y) {
    return lfgpu_ligero_dot_proof_sparse(lp, d_dense, ndense, W2(scale).v, idx, val, nsparse, y);
  }
  static int quadratic(Lig* lp, const E* u, E* y0, E* y2) { return lfgpu_ligero_quadratic_proof(lp, u, y0, y2); }
  static int open(Lig* lp, const size_t* idx, E* req, uint8_t* nonces, uint8_t* path, size_t cap, size_t* npath) {
    return lfgpu_ligero_open(lp, idx, req, nonces, path, cap, npath);
  }
  static int ligero_prove_batch(lfgpu_ctx* c, Lig* const* lp, size_t nb, const E* u_ldt, const E* const* d_dense, size_t ndense, const E* scale,
                                const uint64_t* const* idx, const E* const* val, const size_t* nsparse, const E* u_quad, E* y_ldt, E* y_dot, E* y_q0, E* y_q2) {
    static_assert(sizeof(E) == 16, "E is the uint64_t[2] image the C ABI takes");
    return lfgpu_ligero_prove_batch(c, lp, nb, u_ldt, (const void* const*)d_dense, ndense, (const uint64_t*)scale, idx, (const void* const*)val, nsparse, u_quad,
                                    y_ldt, y_dot, y_q0, y_q2);
  }
  static int ligero_open_batch(lfgpu_ctx* c, Lig* const* lp, size_t nb, const size_t* idx, E* req, uint8_t* nonces, uint8_t* path, size_t cap, size_t* npath) {
    return lfgpu_ligero_open_batch(c, lp, nb, idx, req, nonces, path, cap, npath);
  }
  // LigeroVerifier: rows [0, nwqrow) = [0^r | A_i] extended block -> block_enc, rows nwqrow.. = y_ldt, y_dot, y_quad;
  // ext = those rows at the opened columns.  a_rows(d_T, ld): the caller's inner_product_vector step into the cleared rows.
  template <class ARows>
  static int verifier_ext_with(lfgpu_ctx* c, int field, int k, const lfgpu_ligero_param& p, ARows a_rows, const zkp::ComProof<E>& pr, const size_t* idx,
                               std::vector<E>& ext) {
    const size_t nrows_dev = p.nwqrow + 3, ld = p.block_enc;
    void* dT = nullptr;
    // scratch4: the RS extension below runs its FFT passes through `scratch` / `scratch2` (fft.hip, lch_bs.hip, rs.hip)
    LF_TRY(lf_scratch4(c, (nrows_dev * ld + (size_t)nrows_dev * p.nreq) * 16 + 256, &dT));
    E* d_T = (E*)dT;
    E* d_req = d_T + nrows_dev * ld;
    // only the first dblock columns of a row are inputs: clear them on the device, then strided copies
    LF_HIP(c, hipMemset2DAsync(d_T, ld * 16, 0, p.dblock * 16, nrows_dev, c->stream));
    // inner_product_vector + layout_Aext on the device
    LF_TRY(a_rows(d_T, ld));
    LF_HIP(c, hipMemcpyAsync(d_T + (p.nwqrow + 0) * ld, pr.y_ldt.data(), p.block * 16, hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipMemcpyAsync(d_T + (p.nwqrow + 1) * ld, pr.y_dot.data(), p.dblock * 16, hipMemcpyHostToDevice, c->stream));
    E* yq = d_T + (p.nwqrow + 2) * ld;  // y_quad = y_quad_0 | 0^w | y_quad_2
    LF_HIP(c, hipMemcpyAsync(yq, pr.y_q0.data(), p.r * 16, hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipMemcpyAsync(yq + p.block, pr.y_q2.data(), (p.dblock - p.block) * 16, hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));
    LF_TRY(lf_rs_rows(c, field, k, p.nwqrow + 1, p.block, p.block_enc, d_T, ld));             // A rows and y_ldt
    LF_TRY(lf_rs_rows(c, field, k, 2, p.dblock, p.block_enc, d_T + (p.nwqrow + 1) * ld, ld));  // y_dot, y_quad
    LF_TRY(lfgpu_gather_columns(c, nrows_dev, ld, p.dblock, d_T, idx, p.nreq, d_req));
    ext.resize(nrows_dev * p.nreq);
    LF_HIP(c, hipMemcpyAsync(ext.data(), d_req, ext.size() * 16, hipMemcpyDeviceToHost, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));
    return LFGPU_OK;
  }
  // ZkVerifier: A = scale * EQ over the private inputs + the host-folded sparse terms
  static int verifier_ext(lfgpu_ctx* c, const HostField& F, const lfgpu_circuit_info& I, const lfgpu_ligero_param& p, const E* d_eq, const E& scale,
                          const std::vector<uint64_t>& a_idx, const std::vector<E>& a_val, const zkp::ComProof<E>& pr, const size_t* idx, std::vector<E>& ext) {
    auto a_rows = [&](E* d_T, size_t ld) {
      return lfgpu_ligero_inner_product_rows(c, F.field, p.w, p.r, ld, p.nwqrow, d_eq + I.npub_in, I.ninputs - I.npub_in, W2(scale).v, a_idx.data(), a_val.data(),
                                             a_idx.size(), d_T);
    };
    return verifier_ext_with(c, F.field, 4, p, a_rows, pr, idx, ext);
  }
  // ---- the driver layer (zk_driver.h)
  static constexpr const char *kName = "zk", *kCommitName = "zk_commit", *kCommitBatchName = "zk_commit_batch", *kBatchNewName = "zk_batch_new";
  static constexpr int kLigeroK = 4;
  struct ProverExtra {
    zkp::SubfieldSolver sub;  // GF(2^128): the wire format's subfield runs
    static constexpr void* d_eq = nullptr;  // (the EQ table over the inputs is the context's: eq_store)
    int init(lfgpu_ctx* c, int field, int k, size_t, zkp::Owned*) {
      if (field != LFGPU_FIELD_GF2_128) return LFGPU_OK;
      const GfHostCtx* g = lf_gf_ctx(c, k);
      if (!g) return LFGPU_ERR_ARG;
      sub.build(g);
      return LFGPU_OK;
    }
  };
  static P16 make(lfgpu_ctx* c, int field, int k, const ProverExtra* ex) {
    P16 pol;
    pol.field = field;
    pol.g = lf_gf_ctx(c, k);
    pol.sub = ex ? &ex->sub : nullptr;
    return pol;
  }
  static int ts_ok(lfgpu_ctx*, const lfgpu_transcript_ops*) { return LFGPU_OK; }
  static bool ligero_param_ok(const lfgpu_ligero_param&) { return true; }
  static int eq_store(lfgpu_ctx* c, size_t ninputs, void*, E** d_eq) {
    LF_TRY(zk_eq_reserve(c, ninputs));
    *d_eq = (E*)c->zk_eq;
    return LFGPU_OK;
  }
  // (the per-statement path of prove_batch then finds the context's EQ table in place)
  static int batch_prepare(lfgpu_ctx* c, size_t ninputs) { return zk_eq_reserve(c, ninputs); }
  // the Ligero commit behind lfgpu.h; the witness starts at the private inputs, so the subfield boundary moves down by npub
  static size_t sfb(const lfgpu_circuit_info& I) { return I.subfield_boundary >= I.npub_in ? I.subfield_boundary - I.npub_in : 0; }
  static int lig_commit(lfgpu_ctx* c, const lfgpu_circuit_info& I, const lfgpu_ligero_param& p, const E* W, const size_t* lqc, lfgpu_rng_fn rng, void* user,
                        uint8_t root[32], Lig** out, const lfgpu_comm_ops* shard) {
    if (shard) return lfgpu_ligero_commit_sharded(c, I.field, kLigeroK, &p, W, sfb(I), lqc, rng, user, shard, root, out);
    return lfgpu_ligero_commit(c, I.field, kLigeroK, &p, W, sfb(I), lqc, rng, user, root, out);
  }
  static int lig_commit_batch(lfgpu_ctx* c, const lfgpu_circuit_info& I, const lfgpu_ligero_param& p, size_t nb, const E* const* W, const size_t* lqc,
                              const lfgpu_rng_fn* rng, void* const* users, uint8_t* roots, Lig** out) {
    return lfgpu_ligero_commit_batch(c, I.field, kLigeroK, &p, nb, (const void* const*)W, sfb(I), lqc, rng, users, roots, out);
  }
  static void lig_free(Lig* lp) { lfgpu_ligero_free(lp); }
  // (with a communicator this width records and replays its two random streams in lfgpu_zk_commit instead)
  static int draws_only(lfgpu_ctx*, const lfgpu_ligero_param&, const E*, const size_t*, lfgpu_rng_fn, void*) { return LFGPU_ERR_UNSUPPORTED; }
};
}  // namespace

// ------------------------------------------------------------------ ZkProver
// The ABI's prover handle dispatches on the circuit's field: the record is zkp::Prover<P16> here, or zk256.hip's for Fp256Base.
struct lfgpu_zk_prover {
  lfgpu_ctx* c = nullptr;
  const lfgpu_circuit* C = nullptr;  // compared and passed on, never dereferenced at destruction
  zkp::Prover<P16> p;                // the 16-byte fields
  Zk256* z256 = nullptr;             // Fp256Base circuits: the whole prover lives in zk256.hip
  bool wide() const { return z256 != nullptr; }
  const lfgpu_comm_ops* comm() const { return z256 ? zk256_comm(z256) : p.have_comm ? &p.comm : nullptr; }
  bool have_comm() const { return comm() != nullptr; }
  ~lfgpu_zk_prover() {
    if (z256) zk256_free(z256);
  }
};

extern "C" int lfgpu_zk_prover_new(lfgpu_ctx* c, const lfgpu_circuit* C, size_t rateinv, size_t nreq, size_t block_enc,
                                   lfgpu_zk_prover** out) {
  if (!c || !C || !out || C->c != c) return LFGPU_ERR_ARG;
  std::unique_ptr<lfgpu_zk_prover> zk(new lfgpu_zk_prover());
  zk->c = c;
  zk->C = C;
  if (C->info.field == LFGPU_FIELD_P256) LF_TRY(zk256_new(c, C, rateinv, nreq, block_enc, &zk->z256));
  else LF_TRY(zkp::prover_init<P16>(zk->p, c, C, rateinv, nreq, block_enc));
  *out = zk.release();
  return LFGPU_OK;
}

extern "C" int lfgpu_zk_prover_set_comm(lfgpu_zk_prover* zk, const lfgpu_comm_ops* comm, size_t min_tableau_bytes) {
  if (!zk) return LFGPU_ERR_ARG;
  if (comm && (comm->world < 1 || comm->rank < 0 || comm->rank >= comm->world || !comm->all_gather || !comm->all_to_all || !comm->broadcast))
    return lf_fail(zk->c, LFGPU_ERR_ARG, "zk_prover_set_comm: incomplete communicator");
  if (zk->z256) {
    zk256_set_comm(zk->z256, comm, min_tableau_bytes);
    return LFGPU_OK;
  }
  zk->p.have_comm = comm != nullptr;
  if (comm) {
    zk->p.comm = *comm;
    zk->p.comm_min_bytes = min_tableau_bytes;
  }
  return LFGPU_OK;
}
extern "C" int lfgpu_zk_prover_param(const lfgpu_zk_prover* zk, lfgpu_ligero_param* p) {
  if (!zk || !p) return LFGPU_ERR_ARG;
  if (zk->z256) return zk256_param(zk->z256, p);
  *p = zk->p.st.param;
  return LFGPU_OK;
}

extern "C" int lfgpu_zk_commit(lfgpu_zk_prover* zk, const void* h_W, lfgpu_rng_fn rng, void* rng_user,
                               const lfgpu_transcript_ops* ts, uint8_t root_out[32]) {
  if (!zk || !h_W || !rng || !ts) return LFGPU_ERR_ARG;
  const lfgpu_comm_ops* comm = zk->comm();
  const bool multi = comm && comm->world > 1;
  if (zk->z256) {
    // Fp256Base: with a communicator the ranks share ONE RandomEngine -- rank 0's draws of the whole commit (pads, then the
    // Ligero layout) are recorded and broadcast, the other ranks replay them; zk256_commit then shards the tableau's rows when
    // it is above the threshold (the mdoc signature circuit's 2.5 MB tableau normally stays replicated)
    if (!multi) return zk256_commit(zk->z256, h_W, rng, rng_user, ts, root_out);
    std::vector<uint8_t> stream;
    LF_SCRUB_ON_EXIT(stream);
    alignas(16) unsigned char store[64];
    lfgpu_rng_fn r2 = rng;
    void* u2 = rng_user;
    if (comm->rank == 0) {  // all draws first (no device work, no collective), so that the stream can go out before any collective
      lf_record_rng(rng, rng_user, &stream, &r2, &u2, store);
      const int rc = zk256_commit(zk->z256, h_W, r2, u2, ts, root_out, /*draws_only=*/true);
      if (lf_comm_bcast_blob(comm, stream)) return lf_fail(zk->c, LFGPU_ERR_HIP, "zk_commit: broadcast hook failed");
      if (rc) return rc;
    } else if (lf_comm_bcast_blob(comm, stream)) {
      return lf_fail(zk->c, LFGPU_ERR_HIP, "zk_commit: broadcast hook failed");
    }
    lf_replay_rng(&stream, &r2, &u2, store);
    return zk256_commit(zk->z256, h_W, r2, u2, ts, root_out);
  }
  zkp::Prover<P16>& z = zk->p;
  if (!multi) return zkp::commit<P16>(z, h_W, rng, rng_user, ts, root_out);
  // More than one rank (lfgpu_zk_prover_set_comm): every rank runs this function with the same arguments, but there is ONE
  // RandomEngine -- rank 0's.  Its pad draws are recorded and broadcast, the other ranks replay them (the Ligero commit does
  // the same for its own draws), so all ranks hold the same pads, the same commitment and, with their own copies of the
  // transcript, the same proof.
  const double t0 = now_ms();
  lfgpu_ctx* c = zk->c;
  const lfgpu_circuit_info& I = zk->C->info;
  const bool shard_rows = z.st.param.nrow * z.st.param.block_enc * 16 >= z.comm_min_bytes;
  std::vector<uint8_t> pad_stream;
  LF_SCRUB_ON_EXIT(pad_stream);
  alignas(16) unsigned char rng_store[64];
  if (comm->rank == 0) {
    lf_record_rng(rng, rng_user, &pad_stream, &rng, &rng_user, rng_store);
  } else {
    if (lf_comm_bcast_blob(comm, pad_stream)) return lf_fail(c, LFGPU_ERR_HIP, "zk_commit: broadcast hook failed");
    lf_replay_rng(&pad_stream, &rng, &rng_user, rng_store);
  }
  const P16 pol = z.policy();
  std::vector<elt_t> Wv(z.st.param.nw);  // witness || pads
  LF_SCRUB_ON_EXIT(Wv);
  const size_t pi = zkp::stage_witness(pol, pol.host_field(c), zk->C, z.st, h_W, c->rng_exact != 0, [&](uint8_t* b, size_t n) { rng(rng_user, b, n); }, Wv.data());
  // (rank 0 first sends what the other ranks are waiting for, whatever went wrong here)
  if (comm->rank == 0 && lf_comm_bcast_blob(comm, pad_stream)) return lf_fail(c, LFGPU_ERR_HIP, "zk_commit: broadcast hook failed");
  if (pi != z.st.param.nw) return lf_fail(c, LFGPU_ERR_ASSERT, "zk_commit: witness layout");
  z.drop_commitment();
  if (shard_rows) {
    LF_TRY(P16::lig_commit(c, I, z.st.param, Wv.data(), z.st.lqc.data(), rng, rng_user, z.st.proof.root, &z.lp, comm));
  } else {  // a small tableau stays whole on every rank (replicas): the one random stream still comes from rank 0
    std::vector<uint8_t> lig_stream;
    LF_SCRUB_ON_EXIT(lig_stream);
    alignas(16) unsigned char st2[64];
    lfgpu_rng_fn r2 = rng;
    void* u2 = rng_user;
    if (comm->rank == 0) lf_record_rng(rng, rng_user, &lig_stream, &r2, &u2, st2);
    else {
      if (lf_comm_bcast_blob(comm, lig_stream)) return lf_fail(c, LFGPU_ERR_HIP, "zk_commit: broadcast hook failed");
      lf_replay_rng(&lig_stream, &r2, &u2, st2);
    }
    const int rc = P16::lig_commit(c, I, z.st.param, Wv.data(), z.st.lqc.data(), r2, u2, z.st.proof.root, &z.lp, nullptr);
    // (also after a failed commit: the other ranks are waiting in this broadcast)
    if (comm->rank == 0 && lf_comm_bcast_blob(comm, lig_stream)) return lf_fail(c, LFGPU_ERR_HIP, "zk_commit: broadcast hook failed");
    if (rc) return rc;
  }
  zkp::commit_done(z, ts, root_out, t0);
  return LFGPU_OK;
}

extern "C" int lfgpu_zk_prove(lfgpu_zk_prover* zk, const void* h_W, const lfgpu_transcript_ops* tso, int* ok) {
  if (!zk || !h_W || !tso || !ok) return LFGPU_ERR_ARG;
  return zk->z256 ? zk256_prove(zk->z256, h_W, tso, ok) : zkp::prove<P16>(zk->p, h_W, tso, ok);
}

extern "C" int lfgpu_zk_proof_write(const lfgpu_zk_prover* zk, uint8_t* buf, size_t cap, size_t* nbytes) {
  if (!zk || !nbytes) return LFGPU_ERR_ARG;
  if (zk->z256) return zk256_proof_write(zk->z256, buf, cap, nbytes);
  return zkp::proof_write_cached(zk->c, zk->p.policy(), zk->C, zk->p.st, buf, cap, nbytes);
}

extern "C" int lfgpu_zk_timings(const lfgpu_zk_prover* zk, double ms[6]) {
  if (!zk || !ms) return LFGPU_ERR_ARG;
  if (zk->z256) return zk256_timings(zk->z256, ms);
  memcpy(ms, zk->p.st.ms, sizeof(zk->p.st.ms));
  return LFGPU_OK;
}

extern "C" int lfgpu_zk_prover_free(lfgpu_zk_prover* zk) {
  if (!zk) return LFGPU_ERR_ARG;
  delete zk;
  return LFGPU_OK;
}

// ------------------------------------------------------------------ ZkProver::commit / prove for a batch of provers
// lfgpu_zk_batch (16-byte fields) and lfgpu_zk_batch256 (Fp256Base) are distinct ABI types with one contract: each holds a
// zkp::Batch<P> (zk_driver.h), the second through zk256.hip.  An entry point checks the handles (zkp::check_batch_call) and hands
// the width's records to zkp::prove_batch / zkp::commit_batch, which find what is left to refuse.
struct lfgpu_zk_batch : zkp::Batch<P16> {};
struct lfgpu_zk_batch256 {
  lfgpu_ctx* c = nullptr;
  const lfgpu_circuit* C = nullptr;
  size_t nb_max = 0;
  Zk256Batch* bt = nullptr;
  ~lfgpu_zk_batch256() {
    if (bt) zk256_batch_free(bt);
  }
};
namespace {
std::vector<zkp::Prover<P16>*> records16(lfgpu_zk_prover* const* zk, size_t nb) {
  std::vector<zkp::Prover<P16>*> z(nb);
  for (size_t b = 0; b < nb; ++b) z[b] = &zk[b]->p;
  return z;
}
std::vector<Zk256*> records256(lfgpu_zk_prover* const* zk, size_t nb) {
  std::vector<Zk256*> z(nb);
  for (size_t b = 0; b < nb; ++b) z[b] = zk[b]->z256;
  return z;
}
}  // namespace

extern "C" int lfgpu_zk_batch_new(lfgpu_ctx* c, const lfgpu_circuit* C, size_t nb_max, lfgpu_zk_batch** out) {
  if (!c || !C || !out || C->c != c) return LFGPU_ERR_ARG;
  if (nb_max == 0 || nb_max > LFGPU_SC_BATCH_MAX) return lf_fail(c, LFGPU_ERR_ARG, "zk_batch_new: nb_max must be 1..%d", LFGPU_SC_BATCH_MAX);
  if (C->info.field == LFGPU_FIELD_P256) return lf_fail(c, LFGPU_ERR_UNSUPPORTED, "zk_batch_new: an Fp256Base circuit (lfgpu_zk_batch256_new serves those)");
  std::unique_ptr<lfgpu_zk_batch> bt(new lfgpu_zk_batch());
  LF_TRY(zkp::batch_init<P16>(*bt, c, C, nb_max));
  *out = bt.release();
  return LFGPU_OK;
}
extern "C" int lfgpu_zk_batch256_new(lfgpu_ctx* c, const lfgpu_circuit* C, size_t nb_max, lfgpu_zk_batch256** out) {
  if (!c || !C || !out || C->c != c) return LFGPU_ERR_ARG;
  if (nb_max == 0 || nb_max > LFGPU_SC_BATCH_MAX) return lf_fail(c, LFGPU_ERR_ARG, "zk_batch256_new: nb_max must be 1..%d", LFGPU_SC_BATCH_MAX);
  if (C->info.field != LFGPU_FIELD_P256) return lf_fail(c, LFGPU_ERR_ARG, "zk_batch256_new: the circuit is over a 16-byte field (lfgpu_zk_batch_new serves those)");
  std::unique_ptr<lfgpu_zk_batch256> bt(new lfgpu_zk_batch256());
  bt->c = c;
  bt->C = C;
  bt->nb_max = nb_max;
  LF_TRY(zk256_batch_new(c, C, nb_max, &bt->bt));
  *out = bt.release();
  return LFGPU_OK;
}

extern "C" int lfgpu_zk_prove_batch(lfgpu_zk_batch* bt, lfgpu_zk_prover* const* zk, size_t nb, const void* const* h_W,
                                    const lfgpu_transcript_ops* const* ts, int* ok) {
  if (!bt || !zk || !h_W || !ts || !ok) return LFGPU_ERR_ARG;
  LF_TRY(zkp::check_batch_call("zk_prove_batch", bt->c, bt->C, bt->nb_max, false, zk, nb, h_W, nullptr, ts));
  return zkp::prove_batch<P16>(*bt, records16(zk, nb).data(), nb, h_W, ts, ok);
}
extern "C" int lfgpu_zk_prove_batch256(lfgpu_zk_batch256* bt, lfgpu_zk_prover* const* zk, size_t nb, const void* const* h_W,
                                       const lfgpu_transcript_ops* const* ts, int* ok) {
  if (!bt || !zk || !h_W || !ts || !ok) return LFGPU_ERR_ARG;
  LF_TRY(zkp::check_batch_call("zk_prove_batch256", bt->c, bt->C, bt->nb_max, true, zk, nb, h_W, nullptr, ts));
  return zk256_prove_batch(bt->bt, records256(zk, nb).data(), nb, h_W, ts, ok);
}

extern "C" int lfgpu_zk_commit_batch(lfgpu_zk_batch* bt, lfgpu_zk_prover* const* zk, size_t nb, const void* const* h_W, const lfgpu_rng_fn* rng,
                                     void* const* rng_user, const lfgpu_transcript_ops* const* ts, uint8_t* roots_out) {
  if (!bt || !zk || !h_W || !rng || !ts) return LFGPU_ERR_ARG;
  LF_TRY(zkp::check_batch_call("zk_commit_batch", bt->c, bt->C, bt->nb_max, false, zk, nb, h_W, rng, ts));
  return zkp::commit_batch<P16>(*bt, records16(zk, nb).data(), nb, h_W, rng, rng_user, ts, roots_out);
}
extern "C" int lfgpu_zk_commit_batch256(lfgpu_zk_batch256* bt, lfgpu_zk_prover* const* zk, size_t nb, const void* const* h_W, const lfgpu_rng_fn* rng,
                                        void* const* rng_user, const lfgpu_transcript_ops* const* ts, uint8_t* roots_out) {
  if (!bt || !zk || !h_W || !rng || !ts) return LFGPU_ERR_ARG;
  LF_TRY(zkp::check_batch_call("zk_commit_batch256", bt->c, bt->C, bt->nb_max, true, zk, nb, h_W, rng, ts));
  return zk256_commit_batch(bt->bt, records256(zk, nb).data(), nb, h_W, rng, rng_user, ts, roots_out);
}

extern "C" int lfgpu_zk_batch_free(lfgpu_zk_batch* bt) {
  if (!bt) return LFGPU_ERR_ARG;
  delete bt;
  return LFGPU_OK;
}
extern "C" int lfgpu_zk_batch256_free(lfgpu_zk_batch256* bt) {
  if (!bt) return LFGPU_ERR_ARG;
  delete bt;
  return LFGPU_OK;
}

// ------------------------------------------------------------------ ZkVerifier
// ZkVerifier::recv_commitment + verify over the wire bytes of ZkProof::write: zkp::verify (zk_proto.h); here are the entry
// points and MerkleTreeVerifier::verify_compressed_proof (lib/merkle/merkle_commitment.h:85-99, merkle_tree.h:160-209).

static void hash2(const uint8_t* a, const uint8_t* b, uint8_t out[32]) {  // Digest::hash2: SHA-256(left || right)
  Sha256 s;
  s.update(a, 32);
  s.update(b, 32);
  s.digest(out);
}

// MerkleTreeVerifier::verify_compressed_proof (merkle_tree.h:160-209)
bool lf_merkle_verify(size_t n, const uint8_t root[32], const uint8_t* path, size_t npath, const uint8_t* leaves, const size_t* pos, size_t np) {
  std::vector<uint8_t> layers(2 * n * 32, 0);
  std::vector<bool> defined(2 * n, false), tree(2 * n, false);
  for (size_t ip = 0; ip < np; ++ip) {
    if (pos[ip] >= n) return false;
    tree[pos[ip] + n] = true;
  }
  for (size_t i = n; i-- > 1;) tree[i] = tree[2 * i] || tree[2 * i + 1];
  size_t sz = 0;
  for (size_t i = n; i-- > 1;) {
    if (tree[i]) {
      size_t child = 2 * i;
      if (tree[child]) child = 2 * i + 1;
      if (!tree[child]) {
        if (sz >= npath) return false;
        memcpy(&layers[child * 32], path + 32 * sz++, 32);
        defined[child] = true;
      }
    }
  }
  if (sz != npath) return false;  // the whole proof must be consumed
  for (size_t ip = 0; ip < np; ++ip) {
    memcpy(&layers[(pos[ip] + n) * 32], leaves + 32 * ip, 32);
    defined[pos[ip] + n] = true;
  }
  for (size_t i = n; i-- > 1;)
    if (defined[2 * i] && defined[2 * i + 1]) {
      hash2(&layers[2 * i * 32], &layers[(2 * i + 1) * 32], &layers[i * 32]);
      defined[i] = true;
    }
  return defined[1] && memcmp(root, &layers[32], 32) == 0;
}

static int zk_verify_impl(lfgpu_ctx* c, const lfgpu_circuit* C, size_t rateinv, size_t nreq, size_t block_enc, const uint8_t* proof, size_t proof_len,
                          const void* h_pub, const lfgpu_transcript_ops* tso, bool committed, int* ok, const char** why_out) {
  if (!c || !C || C->c != c || !proof || !tso || !ok || (C->info.npub_in && !h_pub)) return LFGPU_ERR_ARG;
  *ok = 0;
  if (C->info.field == LFGPU_FIELD_P256) return zk256_verify(c, C, rateinv, nreq, block_enc, proof, proof_len, h_pub, tso, committed, ok, why_out);
  const lfgpu_circuit_info& I = C->info;
  lfgpu_ligero_param p{};
  LF_TRY(lfgpu_ligero_param_init(&p, I.field, 4, I.ninputs - I.npub_in + zkp::pad_size(C), C->layers.size(), rateinv, nreq, block_enc));
  if (!lf_gf_ctx(c, 4)) return LFGPU_ERR_ARG;
  auto eq_table = [&](elt_t** d_eq) { return P16::eq_store(c, I.ninputs, nullptr, d_eq); };
  return zkp::verify<P16>(c, C, P16::make(c, I.field, 4, nullptr), p, proof, proof_len, h_pub, tso, committed, eq_table, ok, why_out);
}
extern "C" int lfgpu_zk_verify(lfgpu_ctx* c, const lfgpu_circuit* C, size_t rateinv, size_t nreq, size_t block_enc, const uint8_t* proof,
                               size_t proof_len, const void* h_pub, const lfgpu_transcript_ops* tso, int* ok, const char** why_out) {
  return zk_verify_impl(c, C, rateinv, nreq, block_enc, proof, proof_len, h_pub, tso, false, ok, why_out);
}
extern "C" int lfgpu_zk_verify_committed(lfgpu_ctx* c, const lfgpu_circuit* C, size_t rateinv, size_t nreq, size_t block_enc, const uint8_t* proof,
                                         size_t proof_len, const void* h_pub, const lfgpu_transcript_ops* tso, int* ok, const char** why_out) {
  return zk_verify_impl(c, C, rateinv, nreq, block_enc, proof, proof_len, h_pub, tso, true, ok, why_out);
}

// ------------------------------------------------------------------ LigeroProver::prove / LigeroVerifier::verify on a caller's statement
// zkp::ligero_prove_entry / ligero_verify_entry (zk_driver.h) over the 16-byte fields: the checks of the field and its subfield
// in front, the A step from the term list in ligero.hip.
namespace {
int ligero16_ok(lfgpu_ctx* c, const char* who, int field, int k) {
  if (field != LFGPU_FIELD_GF2_128 && field != LFGPU_FIELD_FP128) return lf_fail(c, LFGPU_ERR_ARG, "%s: field", who);
  if (field == LFGPU_FIELD_GF2_128 && !lf_gf_ctx(c, k)) return lf_fail(c, LFGPU_ERR_ARG, "%s: subfield_log_bits must be 4 or 5", who);
  return LFGPU_OK;
}
}  // namespace

extern "C" int lfgpu_ligero_prove(lfgpu_ligero_prover* lp, const lfgpu_transcript_ops* tso, size_t nl, size_t nllterm, const lfgpu_ligero_llterm* llterm,
                                  const uint8_t hash_of_llterm[32], const size_t* h_lqc, uint8_t* buf, size_t cap, size_t* nbytes) {
  auto pre = [&](const LfLigeroView& v, lfgpu_ligero_prover** lig) {
    *lig = lp;
    LF_TRY(ligero16_ok(v.c, "ligero_prove", v.field, v.k));
    if (!v.whole) return lf_fail(v.c, LFGPU_ERR_UNSUPPORTED, "ligero_prove: the prover must hold the whole tableau on one GPU");
    return (int)LFGPU_OK;
  };
  auto dot = [&](lfgpu_ligero_prover* lig, const std::vector<elt_t>& alphal, const std::vector<elt_t>& alphaq, elt_t* y_dot) {
    const LfLigeroTerms t{llterm, nllterm, alphal.data(), nl, h_lqc, alphaq.data()};
    return lf_ligero_dot_terms(lig, &t, y_dot);
  };
  return zkp::ligero_prove_entry<P16>("ligero_prove", lp, tso, nl, nllterm, llterm, hash_of_llterm, h_lqc, buf, cap, nbytes, pre, dot);
}

extern "C" int lfgpu_ligero_verify(lfgpu_ctx* c, int field, int k, const lfgpu_ligero_param* pp, const uint8_t root[32], const uint8_t* proof, size_t proof_len,
                                   const lfgpu_transcript_ops* tso, size_t nl, size_t nllterm, const lfgpu_ligero_llterm* llterm,
                                   const uint8_t hash_of_llterm[32], const void* h_b, const size_t* h_lqc, int* ok, const char** why_out) {
  auto pre = [&] { return ligero16_ok(c, "ligero_verify", field, k); };
  auto ext = [&](const zkp::ComProof<elt_t>& pr, const std::vector<elt_t>& alphal, const std::vector<elt_t>& alphaq, const size_t* idx, std::vector<elt_t>& out) {
    const LfLigeroTerms t{llterm, nllterm, alphal.data(), nl, h_lqc, alphaq.data()};
    auto a_rows = [&](elt_t* d_T, size_t ld) { return lf_ligero_a_rows_terms(c, field, pp, ld, &t, d_T); };
    return P16::verifier_ext_with(c, field, k, *pp, a_rows, pr, idx, out);
  };
  return zkp::ligero_verify_entry<P16>("ligero_verify", c, field, k, pp, root, proof, proof_len, tso, nl, nllterm, llterm, hash_of_llterm, h_b, h_lqc, ok, why_out,
                                       pre, ext);
}
