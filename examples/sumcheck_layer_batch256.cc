// sumcheck_layer_batch256.cc -- the Fp256Base sumcheck layer (include/lfgpu.h) driven from C++: B statements of one synthetic
// layer go through lfgpu_sumcheck_layer256 one after the other and then through ONE lfgpu_sumcheck_layer_batch256 with the same
// challenges; every evaluation, wc_out, g_out and bound_quad must agree byte for byte.  With --bench N both paths are timed N
// times in alternation; the medians and the spread (min, max) of the repetitions are printed.
// No Python in the loop: a ctypes callback costs about as much as the round trip that is measured.
//
//   g++ -std=c++17 -O2 -Iinclude examples/sumcheck_layer_batch256.cc -Llongfellow-zk_amd -llfgpu -Wl,-rpath,$PWD/longfellow-zk_amd -o sumcheck_layer_batch256
//   ./sumcheck_layer_batch256 LOGV LOGW TERMS NV NW B [--bench N] [--seed S]      (NV / NW = 0: the full powers of two)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
// a canonical element as four words: p = 2^256 - 2^224 + 2^192 + 2^96 - 1 > 2^255, so any value below 2^255 is < p
static void rand_elt(Rng& r, uint64_t out[4]) {
  for (int k = 0; k < 4; ++k) out[k] = r.next();
  out[3] &= 0x7fffffffffffffffull;
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

struct Single {  // callback state of one lfgpu_sumcheck_layer256
  const uint64_t* chal;  // [2 logw][4], in call order
  uint64_t* evals;       // [2 logw][3][4]
  size_t calls;
};
static void round_single(void* user, size_t, size_t, const uint64_t evals[3][4], uint64_t out[4]) {
  Single* s = (Single*)user;
  memcpy(s->evals + 12 * s->calls, evals, 96);
  memcpy(out, s->chal + 4 * s->calls, 32);
  ++s->calls;
}
struct Batch {
  const uint64_t* chal;  // [B][2 logw][4]
  uint64_t* evals;       // [B][2 logw][3][4]
  size_t calls, nrh, bad;
};
static void round_batch(void* user, size_t hand, size_t round, size_t nb, const uint64_t (*evals)[3][4], uint64_t (*out)[4]) {
  Batch* s = (Batch*)user;
  if (s->calls != 2 * round + hand) ++s->bad;  // (round 0, hand 0), (round 0, hand 1), (round 1, hand 0), ...
  for (size_t b = 0; b < nb; ++b) {
    memcpy(s->evals + (b * s->nrh + s->calls) * 12, evals[b], 96);
    memcpy(out[b], s->chal + (b * s->nrh + s->calls) * 4, 32);
  }
  ++s->calls;
}

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: %s LOGV LOGW TERMS NV NW B [--bench N] [--seed S]\n", argv[0]);
    return 2;
  }
  const size_t logv = strtoull(argv[1], nullptr, 10), logw = strtoull(argv[2], nullptr, 10), want_terms = strtoull(argv[3], nullptr, 10);
  size_t nv = strtoull(argv[4], nullptr, 10), nw = strtoull(argv[5], nullptr, 10);
  const size_t B = strtoull(argv[6], nullptr, 10);
  int bench = 0;
  uint64_t seed = 1;
  for (int i = 7; i + 1 < argc; i += 2) {
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
  Rng rng{seed * 0x1000193ull + 11};
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
  std::vector<uint64_t> kvec(4 * nk);
  for (size_t k = 1; k < nk; ++k) rand_elt(rng, &kvec[4 * k]);
  lfgpu_quad* q = nullptr;
  CK(ctx, lfgpu_quad_upload(ctx, LFGPU_FIELD_P256, n, g.data(), h0.data(), h1.data(), vi.data(), nk, kvec.data(), nv, &q));
  // per statement: wires, binding points (statement b's at offset b * logv), alpha, beta, claims, challenges
  std::vector<uint64_t> W(B * nw * 4), G0(B * logv * 4 + 4), G1(B * logv * 4 + 4), alpha(B * 4), beta(B * 4), wc_in(B * 8), chal(B * nrh * 4);
  for (size_t i = 0; i < B * nw; ++i) rand_elt(rng, &W[4 * i]);
  for (size_t i = 0; i < B * logv; ++i) rand_elt(rng, &G0[4 * i]), rand_elt(rng, &G1[4 * i]);
  for (size_t b = 0; b < B; ++b) {
    rand_elt(rng, &alpha[4 * b]);
    rand_elt(rng, &beta[4 * b]);
    rand_elt(rng, &wc_in[8 * b]);
    rand_elt(rng, &wc_in[8 * b + 4]);
  }
  for (size_t i = 0; i < B * nrh; ++i) rand_elt(rng, &chal[4 * i]);
  void* d_W = nullptr;  // [B][nw]: neither call modifies its wires, so both read the same array
  const size_t ldw = nw;
  CK(ctx, lfgpu_malloc(ctx, B * ldw * 32, &d_W));
  CK(ctx, lfgpu_memcpy_h2d(ctx, d_W, W.data(), B * nw * 32));
  std::vector<uint64_t> ev_s(B * nrh * 12), ev_b(B * nrh * 12), wc_s(B * 8), wc_b(B * 8), g_s(B * 2 * logw * 4), g_b(B * 2 * logw * 4), bq_s(B * 4), bq_b(B * 4);
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  auto run_sequential = [&]() -> double {
    CK(ctx, lfgpu_sync(ctx));
    const auto t0 = now();
    for (size_t b = 0; b < B; ++b) {
      Single s{&chal[b * nrh * 4], &ev_s[b * nrh * 12], 0};
      CK(ctx, lfgpu_sumcheck_layer256(q, logv, &G0[b * logv * 4], &G1[b * logv * 4], &alpha[4 * b], &beta[4 * b], logw, nw, (const uint8_t*)d_W + b * ldw * 32,
                                      (const uint64_t(*)[4]) & wc_in[8 * b], round_single, &s, (uint64_t(*)[4]) & wc_s[8 * b], &g_s[b * 2 * logw * 4], &bq_s[4 * b]));
      if (s.calls != nrh) {
        fprintf(stderr, "lfgpu_sumcheck_layer256: %zu callbacks, expected %zu\n", s.calls, nrh);
        exit(1);
      }
    }
    return ms(t0, now());
  };
  auto run_batch = [&]() -> double {
    CK(ctx, lfgpu_sync(ctx));
    Batch s{chal.data(), ev_b.data(), 0, nrh, 0};
    const auto t0 = now();
    CK(ctx, lfgpu_sumcheck_layer_batch256(q, B, logv, G0.data(), G1.data(), alpha.data(), beta.data(), logw, nw, d_W, ldw, wc_in.data(), round_batch, &s,
                                          wc_b.data(), g_b.data(), bq_b.data()));
    const double t = ms(t0, now());
    if (s.calls != nrh || s.bad) {
      fprintf(stderr, "lfgpu_sumcheck_layer_batch256: %zu callbacks (%zu out of order), expected %zu in (round, hand) order\n", s.calls, s.bad, nrh);
      exit(1);
    }
    return t;
  };
  auto check = [&]() {
    if (ev_s == ev_b && wc_s == wc_b && g_s == g_b && bq_s == bq_b) return;
    for (size_t b = 0; b < B; ++b)
      for (size_t k = 0; k < nrh; ++k)
        if (memcmp(&ev_s[(b * nrh + k) * 12], &ev_b[(b * nrh + k) * 12], 96)) {
          fprintf(stderr, "MISMATCH: statement %zu, round-hand %zu: the evaluations differ\n", b, k);
          exit(1);
        }
    fprintf(stderr, "MISMATCH in %s\n", wc_s != wc_b ? "wc_out" : g_s != g_b ? "g_out" : "bound_quad");
    exit(1);
  };
  run_sequential();
  run_batch();
  check();
  // neither path may have touched the wires
  std::vector<uint64_t> Wback(B * nw * 4);
  CK(ctx, lfgpu_memcpy_d2h(ctx, Wback.data(), d_W, B * nw * 32));
  if (Wback != W) {
    fprintf(stderr, "MISMATCH: d_W was modified\n");
    return 1;
  }
  if (bench <= 0) {
    printf("{\"field\": \"p256\", \"logv\": %zu, \"logw\": %zu, \"terms\": %zu, \"nv\": %zu, \"nw\": %zu, \"B\": %zu, \"result\": \"identical\"}\n", logv, logw, n, nv,
           nw, B);
  } else {
    run_sequential();  // warm-up of both paths (the first pass above also recorded the quad's bind shapes)
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
    printf("{\"field\": \"p256\", \"logv\": %zu, \"logw\": %zu, \"terms\": %zu, \"nv\": %zu, \"nw\": %zu, \"B\": %zu, \"bench\": %d, "
           "\"sequential_layer_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, \"batch_layer_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, "
           "\"sequential_us_per_statement\": %.2f, \"batch_us_per_statement\": %.2f, \"batch_over_sequential\": %.4f, \"result\": \"identical\"}\n",
           logv, logw, n, nv, nw, B, bench, ms_s, ts.front(), ts.back(), ms_b, tb.front(), tb.back(), 1e3 * ms_s / (double)B, 1e3 * ms_b / (double)B, ms_b / ms_s);
  }
  lfgpu_free(ctx, d_W);
  lfgpu_quad_free(q);
  lfgpu_shutdown(ctx);
  return 0;
}
