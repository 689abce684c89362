// zk_prove_batch256.cc -- lfgpu_zk_prove_batch256 (include/lfgpu_zk.h) from plain C++: B committed provers of one Fp256Base
// circuit proved through one chain of dispatches, checked against B calls of lfgpu_zk_prove.  The twin of zk_prove_batch.cc
// (the 16-byte fields) with 32-byte witness elements.
//
// B provers are committed with distinct RandomEngine and transcript seeds and proved one by one (lfgpu_zk_prove); the same
// provers are then committed again with the same seeds and proved by ONE lfgpu_zk_prove_batch256.  The B wire images must
// agree byte for byte, and every batched proof must pass lfgpu_zk_verify.  Prints one JSON line; exits non-zero on any
// difference.
// --bench N: after the checked pass one untimed warm-up pass of both, then N passes alternating "B sequential proves" and "one
// batched prove" (commits untimed), medians and ranges per statement in the JSON line, with the constraints and Ligero-prove
// phase times of the last batched pass.
//
//   g++ -std=c++17 -O2 -Iinclude examples/zk_prove_batch256.cc -Llongfellow-zk_amd -llfgpu -Wl,-rpath,$PWD/longfellow-zk_amd -o zk_prove_batch256
//   ./zk_prove_batch256 circuit.lfc1 witness.bin B [--bench N]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "lfgpu_zk.h"

static std::vector<uint8_t> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    fprintf(stderr, "cannot read %s\n", path);
    exit(2);
  }
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
#define CK(ctx, call)                                                          \
  do {                                                                         \
    int rc_ = (call);                                                          \
    if (rc_ != LFGPU_OK) {                                                     \
      fprintf(stderr, "%s -> %d: %s\n", #call, rc_, lfgpu_last_error(ctx));    \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

// RandomEngine of a prover: the built-in AES-CTR PRF keyed by a seed transcript (a real deployment passes its CSPRNG)
static void rng_bytes(void* user, uint8_t* buf, size_t n) { lfgpu_transcript_bytes((lfgpu_transcript*)user, buf, n); }

static const size_t kRate = 7, kNreq = 132;

struct Statement {
  lfgpu_zk_prover* zk = nullptr;
  lfgpu_transcript* ts = nullptr;
  lfgpu_transcript_ops ops{};
};

// (re)commit statement b: RandomEngine seed "rng <b>", transcript seed "ts <b>"
static void commit(lfgpu_ctx* ctx, Statement& s, size_t b, const std::vector<uint8_t>& wit) {
  const std::string rs = "rng " + std::to_string(b), tss = "ts " + std::to_string(b);
  lfgpu_transcript* rng = lfgpu_transcript_new((const uint8_t*)rs.data(), rs.size());
  if (s.ts) lfgpu_transcript_free(s.ts);
  s.ts = lfgpu_transcript_new((const uint8_t*)tss.data(), tss.size());
  lfgpu_transcript_get_ops(s.ts, &s.ops);
  uint8_t root[32];
  CK(ctx, lfgpu_zk_commit(s.zk, wit.data(), rng_bytes, rng, &s.ops, root));
  lfgpu_transcript_free(rng);
}
static std::vector<uint8_t> wire_of(lfgpu_ctx* ctx, const lfgpu_zk_prover* zk) {
  size_t n = 0;
  CK(ctx, lfgpu_zk_proof_write(zk, nullptr, 0, &n));
  std::vector<uint8_t> w(n);
  CK(ctx, lfgpu_zk_proof_write(zk, w.data(), w.size(), &n));
  return w;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s circuit.lfc1 witness.bin B [--bench N]\n", argv[0]);
    return 2;
  }
  const size_t B = (size_t)atoi(argv[3]);
  int bench = 0;
  if (argc > 5 && !strcmp(argv[4], "--bench")) bench = atoi(argv[5]);
  if (B < 1 || B > LFGPU_SC_BATCH_MAX) {
    fprintf(stderr, "B must be 1..%d\n", LFGPU_SC_BATCH_MAX);
    return 2;
  }
  lfgpu_ctx* ctx = nullptr;
  if (lfgpu_init(0, &ctx) != LFGPU_OK) {
    fprintf(stderr, "no MI355X / HIP device: there is no CPU fallback\n");
    return 1;
  }
  const std::vector<uint8_t> lfc1 = slurp(argv[1]), wit = slurp(argv[2]);
  lfgpu_circuit* circ = nullptr;
  CK(ctx, lfgpu_circuit_from_lfc1(ctx, lfc1.data(), lfc1.size(), &circ));
  lfgpu_circuit_info info;
  CK(ctx, lfgpu_circuit_get_info(circ, &info));
  if (info.field != LFGPU_FIELD_P256) {
    fprintf(stderr, "the circuit is over field %d: zk_prove_batch serves the 16-byte fields\n", info.field);
    return 2;
  }
  if (wit.size() != info.ninputs * 32) {
    fprintf(stderr, "witness has %zu bytes, the circuit wants %zu inputs x 32\n", wit.size(), info.ninputs);
    return 2;
  }
  std::vector<Statement> st(B);
  for (size_t b = 0; b < B; ++b) CK(ctx, lfgpu_zk_prover_new(ctx, circ, kRate, kNreq, 0, &st[b].zk));
  lfgpu_zk_batch256* batch = nullptr;
  CK(ctx, lfgpu_zk_batch256_new(ctx, circ, B, &batch));
  std::vector<lfgpu_zk_prover*> zks(B);
  std::vector<const void*> Ws(B, wit.data());
  std::vector<const lfgpu_transcript_ops*> opsv(B);
  std::vector<int> oks(B);
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  auto commit_all = [&] {
    for (size_t b = 0; b < B; ++b) {
      commit(ctx, st[b], b, wit);
      zks[b] = st[b].zk;
      opsv[b] = &st[b].ops;
    }
  };
  auto prove_sequential = [&] {
    const auto t0 = now();
    for (size_t b = 0; b < B; ++b) {
      int ok = 0;
      CK(ctx, lfgpu_zk_prove(st[b].zk, wit.data(), &st[b].ops, &ok));
      oks[b] = ok;
    }
    return ms(t0, now());
  };
  auto prove_batched = [&] {
    const auto t0 = now();
    CK(ctx, lfgpu_zk_prove_batch256(batch, zks.data(), B, Ws.data(), opsv.data(), oks.data()));
    return ms(t0, now());
  };
  auto all_ok = [&](const char* what) {
    for (size_t b = 0; b < B; ++b)
      if (!oks[b]) {
        fprintf(stderr, "%s: the witness does not satisfy the circuit (statement %zu)\n", what, b);
        exit(1);
      }
  };

  // the check: sequential, then batched over the same seeds
  commit_all();
  prove_sequential();
  all_ok("lfgpu_zk_prove");
  std::vector<std::vector<uint8_t>> want(B);
  for (size_t b = 0; b < B; ++b) want[b] = wire_of(ctx, st[b].zk);
  commit_all();
  prove_batched();
  all_ok("lfgpu_zk_prove_batch256");
  bool same = true;
  size_t proof_bytes = 0;
  for (size_t b = 0; b < B; ++b) {
    const std::vector<uint8_t> got = wire_of(ctx, st[b].zk);
    proof_bytes = got.size();
    if (got != want[b]) {
      fprintf(stderr, "statement %zu: the batched proof differs from lfgpu_zk_prove's (%zu vs %zu bytes)\n", b, got.size(), want[b].size());
      same = false;
    }
    if (b && want[b] == want[0]) {
      fprintf(stderr, "statement %zu: same proof as statement 0 -- the seeds do not differ\n", b);
      same = false;
    }
    const std::string tss = "ts " + std::to_string(b);
    lfgpu_transcript* tv = lfgpu_transcript_new((const uint8_t*)tss.data(), tss.size());
    lfgpu_transcript_ops vops;
    lfgpu_transcript_get_ops(tv, &vops);
    int ok = 0;
    const char* why = "";
    CK(ctx, lfgpu_zk_verify(ctx, circ, kRate, kNreq, 0, got.data(), got.size(), wit.data() /*public inputs come first*/, &vops, &ok, &why));
    lfgpu_transcript_free(tv);
    if (!ok) {
      fprintf(stderr, "statement %zu: the verifier rejected the batched proof: %s\n", b, why);
      same = false;
    }
  }
  double ph[6];
  CK(ctx, lfgpu_zk_timings(st[0].zk, ph));

  // the bench: one warm-up pass of both, then alternating passes, commits untimed
  std::vector<double> tseq, tbat;
  if (bench > 0) {
    commit_all();
    prove_sequential();
    commit_all();
    prove_batched();
  }
  for (int r = 0; r < bench; ++r) {
    commit_all();
    tseq.push_back(prove_sequential() / (double)B);
    all_ok("lfgpu_zk_prove");
    commit_all();
    tbat.push_back(prove_batched() / (double)B);
    all_ok("lfgpu_zk_prove_batch256");
  }
  auto med = [](std::vector<double> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
  };
  // the constraints and Ligero-prove phases of the last batched pass: with the batched Ligero prove (the default) they are the
  // batch's phase times, the same for every member; with LFGPU_LIGERO_PROVE_BATCH256=0 statement 0's own
  double pl[6], pz[6];
  CK(ctx, lfgpu_zk_timings(st[0].zk, pl));
  CK(ctx, lfgpu_zk_timings(st[B - 1].zk, pz));
  const bool shared = B > 1 && pl[4] == pz[4] && pl[5] == pz[5];
  auto lo = [](const std::vector<double>& v) { return v.empty() ? 0.0 : *std::min_element(v.begin(), v.end()); };
  auto hi = [](const std::vector<double>& v) { return v.empty() ? 0.0 : *std::max_element(v.begin(), v.end()); };
  printf("{\"B\": %zu, \"field\": %d, \"layers\": %zu, \"terms\": %zu, \"proof_bytes\": %zu, \"batch_equals_sequential\": %s, \"bench_passes\": %d, "
         "\"sequential_ms_per_statement\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
         "\"batched_ms_per_statement\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}, "
         "\"batch_phases_ms\": {\"prove\": %.3f, \"eval_circuit\": %.3f, \"sumcheck\": %.3f, \"constraints_0\": %.3f, \"ligero_prove_0\": %.3f}, "
         "\"last_batched_pass_ms\": {\"constraints\": %.3f, \"ligero_prove\": %.3f, \"shared_by_all_members\": %s}}\n",
         B, info.field, info.nl, info.nterms, proof_bytes, same ? "true" : "false", bench, med(tseq), lo(tseq), hi(tseq), med(tbat), lo(tbat), hi(tbat), ph[1], ph[2],
         ph[3], ph[4], ph[5], pl[4], pl[5], shared ? "true" : "false");
  for (size_t b = 0; b < B; ++b) {
    lfgpu_transcript_free(st[b].ts);
    lfgpu_zk_prover_free(st[b].zk);
  }
  lfgpu_zk_batch256_free(batch);
  lfgpu_circuit_free(circ);
  lfgpu_shutdown(ctx);
  return same ? 0 : 1;
}
