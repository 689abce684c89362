// sumcheck_layer_batch.cc -- lfgpu_sumcheck_layer_batch (include/lfgpu.h, K14) driven from C++: B statements of one synthetic
// layer go through lfgpu_sumcheck_layer one after the other and then through ONE batched call with the same challenges; every
// evaluation, wc_out, g_out and bound_quad must agree byte for byte.  With --bench N the two paths are timed in alternation.
// No Python in the loop: a ctypes callback costs about as much as the round trip that is measured.
//
//   g++ -std=c++17 -O2 -Iinclude examples/sumcheck_layer_batch.cc -Llongfellow-zk_amd -llfgpu -Wl,-rpath,$PWD/longfellow-zk_amd -o sumcheck_layer_batch
//   ./sumcheck_layer_batch gf|fp LOGV LOGW TERMS NV NW B [--bench N] [--seed S]      (NV / NW = 0: the full powers of two)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lfgpu.h"

#define CK(ctx, call)                                                       \
  do {                                                                      \
    int rc_ = (call);                                                       \
    if (rc_ != LFGPU_OK) {                                                  \
      fprintf(stderr, "%s -> %d: %s\n", #call, rc_, lfgpu_last_error(ctx)); \
      exit(1);                                                              \
    }                                                                       \
  } while (0)

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return next() % n; }
};
// a field element as two words; Fp128 (p = 2^128 - 2^108 + 1): any value with the high word below 2^64 - 2^44 is < p
static void rand_elt(Rng& r, bool fp, uint64_t out[2]) {
  out[0] = r.next();
  out[1] = r.next();
  if (fp)
    while (out[1] >= 0xfffff00000000000ull) out[1] = r.next();
}
static uint64_t morton(uint32_t a, uint32_t b) {
  uint64_t m = 0;
  for (int i = 0; i < 32; ++i) m |= ((uint64_t)((a >> i) & 1) << (2 * i)) | ((uint64_t)((b >> i) & 1) << (2 * i + 1));
  return m;
}
struct Term {
  uint64_t m;
  uint32_t g, h0, h1;
  bool operator<(const Term& o) const { return m != o.m ? m < o.m : g < o.g; }
  bool operator==(const Term& o) const { return m == o.m && g == o.g; }
};

struct Single {  // callback state of one lfgpu_sumcheck_layer
  const uint64_t* chal;  // [2 logw][2], in call order
  uint64_t* evals;       // [2 logw][3][2]
  size_t calls;
};
static void round_single(void* user, size_t, size_t, const uint64_t evals[3][2], uint64_t out[2]) {
  Single* s = (Single*)user;
  memcpy(s->evals + 6 * s->calls, evals, 48);
  out[0] = s->chal[2 * s->calls];
  out[1] = s->chal[2 * s->calls + 1];
  ++s->calls;
}
struct Batch {
  const uint64_t* chal;  // [B][2 logw][2]
  uint64_t* evals;       // [B][2 logw][3][2]
  size_t calls, nrh, bad;
};
static void round_batch(void* user, size_t hand, size_t round, size_t nb, const uint64_t (*evals)[3][2], uint64_t (*out)[2]) {
  Batch* s = (Batch*)user;
  if (s->calls != 2 * round + hand) ++s->bad;  // (round 0, hand 0), (round 0, hand 1), (round 1, hand 0), ...
  for (size_t b = 0; b < nb; ++b) {
    memcpy(s->evals + (b * s->nrh + s->calls) * 6, evals[b], 48);
    out[b][0] = s->chal[(b * s->nrh + s->calls) * 2];
    out[b][1] = s->chal[(b * s->nrh + s->calls) * 2 + 1];
  }
  ++s->calls;
}

int main(int argc, char** argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: %s gf|fp LOGV LOGW TERMS NV NW B [--bench N] [--seed S]\n", argv[0]);
    return 2;
  }
  const bool fp = !strcmp(argv[1], "fp");
  if (!fp && strcmp(argv[1], "gf")) {
    fprintf(stderr, "field must be gf or fp\n");
    return 2;
  }
  const int field = fp ? LFGPU_FIELD_FP128 : LFGPU_FIELD_GF2_128;
  const size_t logv = strtoull(argv[2], nullptr, 10), logw = strtoull(argv[3], nullptr, 10), want_terms = strtoull(argv[4], nullptr, 10);
  size_t nv = strtoull(argv[5], nullptr, 10), nw = strtoull(argv[6], nullptr, 10);
  const size_t B = strtoull(argv[7], nullptr, 10);
  int bench = 0;
  uint64_t seed = 1;
  for (int i = 8; i + 1 < argc; i += 2) {
    if (!strcmp(argv[i], "--bench")) bench = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "--seed")) seed = strtoull(argv[i + 1], nullptr, 10);
  }
  if (logv > 28 || logw > 28 || logw == 0 || want_terms == 0) {
    fprintf(stderr, "LOGV <= 28, 1 <= LOGW <= 28, TERMS >= 1\n");
    return 2;
  }
  if (!nv) nv = (size_t)1 << logv;
  if (!nw) nw = (size_t)1 << logw;
  if (nv > ((size_t)1 << logv) || nw > ((size_t)1 << logw) || B == 0 || B > LFGPU_SC_BATCH_MAX) {
    fprintf(stderr, "NV <= 2^LOGV, NW <= 2^LOGW, 1 <= B <= %d\n", LFGPU_SC_BATCH_MAX);
    return 2;
  }
  lfgpu_ctx* ctx = nullptr;
  if (lfgpu_init(0, &ctx) != LFGPU_OK) {
    fprintf(stderr, "no MI355X / HIP device: there is no CPU fallback\n");
    return 1;
  }
  // the layer in canonical order (EQuad::canonicalize): unique (h0 <= h1, g), sorted by Morton(h0, h1), then g
  Rng rng{seed * 0x1000193ull + (fp ? 7 : 3)};
  std::vector<Term> terms;
  // (at most half of the nv * nw (nw + 1) / 2 distinct triples, so that drawing them terminates quickly)
  const double half_space = 0.25 * (double)nv * (double)nw * (double)(nw + 1) + 1;
  const size_t cap = (double)want_terms < half_space ? want_terms : (size_t)half_space;
  while (terms.size() < cap) {
    const size_t need = cap - terms.size();
    for (size_t i = 0; i < need + need / 8 + 8; ++i) {
      const uint32_t a = (uint32_t)rng.below(nw), b = (uint32_t)rng.below(nw);
      Term t{0, (uint32_t)rng.below(nv), std::min(a, b), std::max(a, b)};
      t.m = morton(t.h0, t.h1);
      terms.push_back(t);
    }
    std::sort(terms.begin(), terms.end());
    terms.erase(std::unique(terms.begin(), terms.end()), terms.end());
    if (terms.size() > cap) {  // drop the surplus evenly, the order stays canonical
      std::vector<Term> keep;
      keep.reserve(cap);
      for (size_t i = 0; i < cap; ++i) keep.push_back(terms[i * terms.size() / cap]);
      terms.swap(keep);
    }
  }
  const size_t n = terms.size(), nk = 9, nrh = 2 * logw;
  std::vector<uint32_t> g(n), h0(n), h1(n), vi(n);
  for (size_t i = 0; i < n; ++i) {
    g[i] = terms[i].g;
    h0[i] = terms[i].h0;
    h1[i] = terms[i].h1;
    vi[i] = 1 + (uint32_t)rng.below(nk - 1);
  }
  std::vector<uint64_t> kvec(2 * nk);
  for (size_t k = 1; k < nk; ++k) rand_elt(rng, fp, &kvec[2 * k]);
  lfgpu_quad* q = nullptr;
  CK(ctx, lfgpu_quad_upload(ctx, field, n, g.data(), h0.data(), h1.data(), vi.data(), nk, kvec.data(), nv, &q));
  // per statement: wires, binding points, alpha, beta, claims, challenges
  const size_t lv = std::max<size_t>(logv, 1);
  std::vector<uint64_t> W(B * nw * 2), G0(B * lv * 2), G1(B * lv * 2), alpha(B * 2), beta(B * 2), wc_in(B * 4), chal(B * nrh * 2);
  for (size_t i = 0; i < B * nw; ++i) rand_elt(rng, fp, &W[2 * i]);
  for (size_t i = 0; i < B * lv; ++i) rand_elt(rng, fp, &G0[2 * i]), rand_elt(rng, fp, &G1[2 * i]);
  for (size_t b = 0; b < B; ++b) {
    rand_elt(rng, fp, &alpha[2 * b]);
    rand_elt(rng, fp, &beta[2 * b]);
    rand_elt(rng, fp, &wc_in[4 * b]);
    rand_elt(rng, fp, &wc_in[4 * b + 2]);
  }
  for (size_t i = 0; i < B * nrh; ++i) rand_elt(rng, fp, &chal[2 * i]);
  // (the library reads statement b's points at offset b * logv: pack them so when logv = 0 left room for one element each)
  std::vector<uint64_t> G0p(B * lv * 2), G1p(B * lv * 2);
  for (size_t b = 0; b < B; ++b)
    for (size_t l = 0; l < logv; ++l) {
      memcpy(&G0p[(b * logv + l) * 2], &G0[(b * lv + l) * 2], 16);
      memcpy(&G1p[(b * logv + l) * 2], &G1[(b * lv + l) * 2], 16);
    }
  void* d_Ws = nullptr;  // the wires of the sequential calls, [B][nw]
  void* d_Wb = nullptr;  // ... and of the batched call, [B][ldw]
  const size_t ldw = nw;
  CK(ctx, lfgpu_malloc(ctx, B * nw * 16, &d_Ws));
  CK(ctx, lfgpu_malloc(ctx, B * ldw * 16, &d_Wb));
  std::vector<uint64_t> ev_s(B * nrh * 6), ev_b(B * nrh * 6), wc_s(B * 4), wc_b(B * 4), g_s(B * 2 * logw * 2), g_b(B * 2 * logw * 2), bq_s(B * 2), bq_b(B * 2);
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  // both paths consume their wires: refill (untimed) before every pass
  auto run_sequential = [&]() -> double {
    CK(ctx, lfgpu_memcpy_h2d(ctx, d_Ws, W.data(), B * nw * 16));
    CK(ctx, lfgpu_sync(ctx));
    const auto t0 = now();
    for (size_t b = 0; b < B; ++b) {
      Single s{&chal[b * nrh * 2], &ev_s[b * nrh * 6], 0};
      CK(ctx, lfgpu_sumcheck_layer(q, logv, &G0p[b * logv * 2], &G1p[b * logv * 2], &alpha[2 * b], &beta[2 * b], logw, nw, (uint8_t*)d_Ws + b * nw * 16,
                                   (const uint64_t(*)[2]) & wc_in[4 * b], round_single, &s, (uint64_t(*)[2]) & wc_s[4 * b], &g_s[b * 2 * logw * 2], &bq_s[2 * b]));
      if (s.calls != nrh) {
        fprintf(stderr, "lfgpu_sumcheck_layer: %zu callbacks, expected %zu\n", s.calls, nrh);
        exit(1);
      }
    }
    return ms(t0, now());
  };
  auto run_batch = [&]() -> double {
    CK(ctx, lfgpu_memcpy_h2d(ctx, d_Wb, W.data(), B * nw * 16));
    CK(ctx, lfgpu_sync(ctx));
    Batch s{chal.data(), ev_b.data(), 0, nrh, 0};
    const auto t0 = now();
    CK(ctx, lfgpu_sumcheck_layer_batch(q, B, logv, G0p.data(), G1p.data(), alpha.data(), beta.data(), logw, nw, d_Wb, ldw, wc_in.data(), round_batch, &s,
                                       wc_b.data(), g_b.data(), bq_b.data()));
    const double t = ms(t0, now());
    if (s.calls != nrh || s.bad) {
      fprintf(stderr, "lfgpu_sumcheck_layer_batch: %zu callbacks (%zu out of order), expected %zu in (round, hand) order\n", s.calls, s.bad, nrh);
      exit(1);
    }
    return t;
  };
  auto check = [&]() {
    const bool ok = ev_s == ev_b && wc_s == wc_b && g_s == g_b && bq_s == bq_b;
    if (!ok) {
      for (size_t b = 0; b < B; ++b)
        for (size_t k = 0; k < nrh; ++k)
          if (memcmp(&ev_s[(b * nrh + k) * 6], &ev_b[(b * nrh + k) * 6], 48)) {
            fprintf(stderr, "MISMATCH: statement %zu, round-hand %zu: the evaluations differ\n", b, k);
            exit(1);
          }
      fprintf(stderr, "MISMATCH in %s\n", wc_s != wc_b ? "wc_out" : g_s != g_b ? "g_out" : "bound_quad");
      exit(1);
    }
  };
  run_sequential();
  run_batch();
  check();
  if (bench <= 0) {
    printf("{\"field\": \"%s\", \"logv\": %zu, \"logw\": %zu, \"terms\": %zu, \"nv\": %zu, \"nw\": %zu, \"B\": %zu, \"batch_equals_sequential\": true}\n", argv[1],
           logv, logw, n, nv, nw, B);
  } else {
    run_sequential();  // warm-up of both paths (the first pass above also recorded the quad's bind shapes / grid offsets)
    run_batch();
    std::vector<double> ts, tb;
    for (int i = 0; i < bench; ++i) {
      ts.push_back(run_sequential());
      tb.push_back(run_batch());
    }
    check();
    std::sort(ts.begin(), ts.end());
    std::sort(tb.begin(), tb.end());
    const double ms_s = ts[ts.size() / 2], ms_b = tb[tb.size() / 2];
    printf("{\"field\": \"%s\", \"logv\": %zu, \"logw\": %zu, \"terms\": %zu, \"nv\": %zu, \"nw\": %zu, \"B\": %zu, \"bench\": %d, "
           "\"sequential_layer_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, \"batch_layer_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, "
           "\"sequential_us_per_statement\": %.2f, \"batch_us_per_statement\": %.2f, \"batch_over_sequential\": %.4f, \"batch_equals_sequential\": true}\n",
           argv[1], logv, logw, n, nv, nw, B, bench, ms_s, ts.front(), ts.back(), ms_b, tb.front(), tb.back(), 1e3 * ms_s / (double)B, 1e3 * ms_b / (double)B,
           ms_b / ms_s);
  }
  lfgpu_free(ctx, d_Ws);
  lfgpu_free(ctx, d_Wb);
  lfgpu_quad_free(q);
  lfgpu_shutdown(ctx);
  return 0;
}
