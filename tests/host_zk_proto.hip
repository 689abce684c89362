// Host-only harness of tests/test_zk_proto_host.py: the parts of csrc/zk_proto.h that need no device context (transcript
// view, ZkProof::write / read, inner_product_sparse, stage_witness) behind a small C ABI.  Compiled with hipcc --cuda-host-only and linked
// against liblfgpu.so for the host helpers the header calls (field inverses, the GF(2^128) constants).
// Elements cross this ABI as their to_bytes_field images (canonical little-endian values), never in Montgomery form.
#include "../longfellow-zk_amd/csrc/zk_proto.h"

namespace {
struct Gf {  // GF(2^128): the subfield tables without a context
  GfHostCtx g;
  zkp::SubfieldSolver sub;
  Gf() {
    lf_gf_ctx_build(&g, 4);
    sub.build(&g);
  }
};
zkp::Wire16 wire16(int field) {
  zkp::Wire16 w;
  w.field = field;
  if (field == LFGPU_FIELD_GF2_128) {
    static const Gf gf;
    w.g = &gf.g;
    w.sub = &gf.sub;
  }
  return w;
}
// f(policy, host field) for the field id; the prime fields' host fields need no context, GF(2^128)'s only the constants of one
template <class Fn>
int with_field(int field, Fn f) {
  if (field == LFGPU_FIELD_P256) return f(zkp::Wire32(), F256());
  if (field == LFGPU_FIELD_FP128) return f(wire16(field), HostField(nullptr, field));
  static lfgpu_ctx no_device;  // (never initialised: lf_gf_ctx builds its host tables in place)
  return f(wire16(field), HostField(&no_device, field));
}
template <class Fn>
int with_wire(int field, Fn f) {
  if (field == LFGPU_FIELD_P256) return f(zkp::Wire32());
  return f(wire16(field));
}
template <class P>
bool get(const P& pol, const uint8_t* b, size_t n, std::vector<typename P::E>& v) {
  v.assign(n, P::zero());
  bool ok = true;
  for (size_t i = 0; i < n; ++i) ok &= pol.of_bytes(b + P::kBytes * i, v[i]);
  return ok;
}
template <class P>
void put(const P& pol, const std::vector<typename P::E>& v, uint8_t* b) {
  for (size_t i = 0; i < v.size(); ++i) pol.to_bytes(v[i], b + P::kBytes * i);
}
void layers_of(lfgpu_circuit& C, const size_t* logw, size_t nl) {
  for (size_t i = 0; i < nl; ++i) C.layers.push_back({logw[i], (size_t)1 << logw[i], 1, nullptr});
}
}  // namespace

extern "C" {
// sc: per layer hp[0][0 .. 2 logw) | hp[1][0 .. 2 logw) | wc[0] | wc[1]; the other members as in zkp::ProofBody
struct hzp_proof {
  uint8_t root[32];
  uint8_t *sc, *y_ldt, *y_dot, *y_q0, *y_q2, *req, *nonces, *path;
  size_t npath;
};

// ZkProof::write of the proof in `in` (nreq * nrow opened elements); 0, or -1 when an input element is not canonical
int hzp_write(int field, const size_t* logw, size_t nl, const lfgpu_ligero_param* p, const hzp_proof* in, uint8_t* out, size_t cap, size_t* nbytes) {
  return with_wire(field, [&](auto pol) {
    using P = decltype(pol);
    lfgpu_circuit C;
    layers_of(C, logw, nl);
    zkp::ProofBody<typename P::E> pr;
    memcpy(pr.root, in->root, 32);
    pr.sc.assign(nl, {});
    const uint8_t* s = in->sc;
    bool ok = true;
    for (size_t ly = 0; ly < nl; ++ly) {
      std::vector<typename P::E> wc;
      ok &= get(pol, s, 2 * logw[ly], pr.sc[ly].hp[0]) && get(pol, s + 2 * logw[ly] * P::kBytes, 2 * logw[ly], pr.sc[ly].hp[1]) &&
            get(pol, s + 4 * logw[ly] * P::kBytes, 2, wc);
      pr.sc[ly].wc[0] = wc[0];
      pr.sc[ly].wc[1] = wc[1];
      s += (4 * logw[ly] + 2) * P::kBytes;
    }
    ok &= get(pol, in->y_ldt, p->block, pr.y_ldt) && get(pol, in->y_dot, p->dblock, pr.y_dot) && get(pol, in->y_q0, p->r, pr.y_q0) &&
          get(pol, in->y_q2, p->dblock - p->block, pr.y_q2) && get(pol, in->req, p->nreq * p->nrow, pr.req);
    if (!ok) return -1;
    pr.nonces.assign(in->nonces, in->nonces + 32 * p->nreq);
    pr.path.assign(in->path, in->path + 32 * in->npath);
    pr.npath = in->npath;
    std::vector<uint8_t> o;
    zkp::proof_write(pol, &C, pr, o);
    *nbytes = o.size();
    if (o.size() > cap) return -1;
    memcpy(out, o.data(), o.size());
    return 0;
  });
}

// ZkProof::read: 1 and the proof in `out` (buffers of the sizes p fixes; path: nreq * mc_pathlen digests), or 0 when refused
int hzp_read(int field, const size_t* logw, size_t nl, const lfgpu_ligero_param* p, const uint8_t* buf, size_t len, hzp_proof* out) {
  return with_wire(field, [&](auto pol) {
    using P = decltype(pol);
    lfgpu_circuit C;
    layers_of(C, logw, nl);
    zkp::ProofBody<typename P::E> pr;
    if (!zkp::proof_read(pol, &C, *p, buf, len, pr)) return 0;
    memcpy(out->root, pr.root, 32);
    uint8_t* s = out->sc;
    for (size_t ly = 0; ly < nl; ++ly) {
      put(pol, pr.sc[ly].hp[0], s);
      put(pol, pr.sc[ly].hp[1], s + 2 * logw[ly] * P::kBytes);
      put(pol, {pr.sc[ly].wc[0], pr.sc[ly].wc[1]}, s + 4 * logw[ly] * P::kBytes);
      s += (4 * logw[ly] + 2) * P::kBytes;
    }
    put(pol, pr.y_ldt, out->y_ldt);
    put(pol, pr.y_dot, out->y_dot);
    put(pol, pr.y_q0, out->y_q0);
    put(pol, pr.y_q2, out->y_q2);
    put(pol, pr.req, out->req);
    memcpy(out->nonces, pr.nonces.data(), pr.nonces.size());
    memcpy(out->path, pr.path.data(), pr.path.size());
    out->npath = pr.npath;
    return 1;
  });
}

// inner_product_sparse over na linear terms (constraint a_c, witness index a_w, coefficient a_k), alphal[nalphal], lqc[3 nq],
// alphaq[3 nq]; idx_out / val_out have room for na + 6 nq entries
int hzp_inner_product_sparse(int field, const lfgpu_ligero_param* p, size_t na, const size_t* a_c, const size_t* a_w, const uint8_t* a_k, size_t nalphal,
                             const uint8_t* alphal, const size_t* lqc, const uint8_t* alphaq, uint64_t* idx_out, uint8_t* val_out, size_t* n_out) {
  return with_field(field, [&](auto pol, const auto& F) {
    using P = decltype(pol);
    using E = typename P::E;
    std::vector<E> k, al, aq, val;
    if (!get(pol, a_k, na, k) || !get(pol, alphal, nalphal, al) || !get(pol, alphaq, 3 * p->nq, aq)) return -1;
    std::vector<zkp::LinTerm<E>> a(na);
    for (size_t i = 0; i < na; ++i) a[i] = {a_c[i], a_w[i], k[i]};
    std::vector<uint64_t> idx;
    zkp::inner_product_sparse<P>(F, *p, a, al, std::vector<size_t>(lqc, lqc + 3 * p->nq), aq, idx, val);
    std::copy(idx.begin(), idx.end(), idx_out);
    put(pol, val, val_out);
    *n_out = idx.size();
    return 0;
  });
}

// A RandomEngine that hands out `stream` in order (zeros and *over = true past its end) and records the size of every call
struct ScriptedRng {
  const uint8_t* stream;
  size_t len, *calls, cap, ncalls = 0, pos = 0;
  bool over = false;
  void operator()(uint8_t* b, size_t n) {
    if (ncalls < cap) calls[ncalls] = n;
    ++ncalls;
    if (n > len - pos) {
      over = true;
      memset(b, 0, n);
      return;
    }
    memcpy(b, stream + pos, n);
    pos += n;
  }
};
// zkp::stage_witness for a circuit of nl layers (logw[]) with npub public among ninputs inputs (h_W: all of them) over the
// scripted engine: the staged vector (n_witness + pad_size elements), lqc[3 nl], the returned length, the engine's call sizes.
// bulk_model != 0 (Fp256Base): not stage_witness but ONE h256_sample_many over the same stream, placed by pad_layout.
int hzp_stage_witness(int field, const size_t* logw, size_t nl, size_t npub, size_t ninputs, const uint8_t* h_W, int exact, int bulk_model, const uint8_t* stream,
                      size_t stream_len, size_t* calls, size_t calls_cap, size_t* ncalls, uint8_t* Wv_out, size_t* lqc_out, size_t* len_out) {
  return with_field(field, [&](auto pol, const auto& F) {
    using P = decltype(pol);
    using E = typename P::E;
    lfgpu_circuit C;
    layers_of(C, logw, nl);
    C.info.npub_in = npub;
    C.info.ninputs = ninputs;
    zkp::ProverState<P> st;
    st.init(&C);
    std::vector<E> W, Wv(st.n_witness + st.pad_size, P::zero());
    if (!get(pol, h_W, ninputs, W)) return -1;
    ScriptedRng rng{stream, stream_len, calls, calls_cap};
    if constexpr (P::kBytes == 32) {
      if (bulk_model) {
        std::vector<E> pads(st.pad_size - nl);
        h256_sample_many(pads.data(), pads.size(), [&](uint8_t* b, size_t n) { rng(b, n); });
        size_t pd = 0;
        memcpy(Wv.data(), W.data() + npub, st.n_witness * 32);
        *len_out = zkp::pad_layout<P>(F, &C, st.n_witness, st.lqc, [&] { return pads[pd++]; }, &st.pad, Wv.data());
      }
    }
    if (!bulk_model) *len_out = zkp::stage_witness(pol, F, &C, st, W.data(), exact != 0, [&](uint8_t* b, size_t n) { rng(b, n); }, Wv.data());
    *ncalls = rng.ncalls;
    put(pol, Wv, Wv_out);
    std::copy(st.lqc.begin(), st.lqc.end(), lqc_out);
    return rng.over ? -2 : 0;
  });
}

// the transcript view over the caller's hooks
size_t hzp_nat(int field, const lfgpu_transcript_ops* ops, size_t n) {
  size_t r = 0;
  with_wire(field, [&](auto pol) {
    r = zkp::Ts<decltype(pol)>{&pol, ops, ops->user}.nat(n);
    return 0;
  });
  return r;
}
void hzp_choose(int field, const lfgpu_transcript_ops* ops, size_t n, size_t k, size_t* res) {
  with_wire(field, [&](auto pol) {
    zkp::Ts<decltype(pol)>{&pol, ops, ops->user}.choose(n, k, res);
    return 0;
  });
}
int hzp_write_array(int field, const lfgpu_transcript_ops* ops, const uint8_t* elts, size_t n) {
  return with_wire(field, [&](auto pol) {
    std::vector<typename decltype(pol)::E> v;
    if (!get(pol, elts, n, v)) return -1;
    zkp::Ts<decltype(pol)>{&pol, ops, ops->user}.write_array(v.data(), n);
    return 0;
  });
}
int hzp_write_elt(int field, const lfgpu_transcript_ops* ops, const uint8_t* elt) {
  return with_wire(field, [&](auto pol) {
    std::vector<typename decltype(pol)::E> v;
    if (!get(pol, elt, 1, v)) return -1;
    zkp::Ts<decltype(pol)>{&pol, ops, ops->user}.write_elt(v[0]);
    return 0;
  });
}
}  // extern "C"
