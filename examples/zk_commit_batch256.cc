// zk_commit_batch256.cc -- lfgpu_zk_commit_batch256 (include/lfgpu_zk.h) from plain C++: the commits of B statements of one
// Fp256Base circuit (field id 1, 32-byte elements) through one chain of dispatches, checked against B calls of lfgpu_zk_commit.
// The twin of zk_commit_batch.cc, which does the same for the 16-byte fields.
//
// Set A of B provers is committed one by one (lfgpu_zk_commit), set B by ONE lfgpu_zk_commit_batch256 with the same RandomEngine
// and transcript seeds.  The B roots must agree; both sets then go through lfgpu_zk_prove_batch256, the B wire images must agree
// byte for byte, and every proof of the batched set must pass lfgpu_zk_verify.  Prints one JSON line; exits non-zero on any
// difference.
// --bench N: N passes on fresh seeds alternating "B sequential commits" and "one batched commit", then N passes alternating
// the two followed by lfgpu_zk_prove_batch256 (the whole pipeline); medians and ranges per statement in the JSON line.  The host
// clock runs around calls that end in a stream synchronise.
//
//   g++ -std=c++17 -O2 -Iinclude examples/zk_commit_batch256.cc -Llongfellow-zk_amd -llfgpu -Wl,-rpath,$PWD/longfellow-zk_amd -o zk_commit_batch256
//   ./zk_commit_batch256 circuit.lfc1 witness.bin B [--bench N]
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

static const size_t kRate = 7, kNreq = 132;  // the mdoc signature circuit's

struct Set {  // B provers with their transcripts and RandomEngines
  std::vector<lfgpu_zk_prover*> zk;
  std::vector<lfgpu_transcript*> ts, rng;
  std::vector<lfgpu_transcript_ops> ops;
  std::vector<const lfgpu_transcript_ops*> opsp;
  std::vector<lfgpu_rng_fn> fns;
  std::vector<void*> users;
  std::vector<uint8_t> roots;
  explicit Set(size_t B) : zk(B), ts(B, nullptr), rng(B, nullptr), ops(B), opsp(B), fns(B, rng_bytes), users(B), roots(32 * B) {}
  // statement b of pass `pass`: RandomEngine seed "rng <pass> <b>", transcript seed "ts <pass> <b>"
  void reseed(int pass) {
    for (size_t b = 0; b < zk.size(); ++b) {
      const std::string rs = "rng " + std::to_string(pass) + " " + std::to_string(b), tss = "ts " + std::to_string(pass) + " " + std::to_string(b);
      if (ts[b]) lfgpu_transcript_free(ts[b]);
      if (rng[b]) lfgpu_transcript_free(rng[b]);
      rng[b] = lfgpu_transcript_new((const uint8_t*)rs.data(), rs.size());
      ts[b] = lfgpu_transcript_new((const uint8_t*)tss.data(), tss.size());
      lfgpu_transcript_get_ops(ts[b], &ops[b]);
      opsp[b] = &ops[b];
      users[b] = rng[b];
    }
  }
};

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
    fprintf(stderr, "the circuit is over field %d: zk_commit_batch serves the 16-byte fields\n", info.field);
    return 2;
  }
  if (wit.size() != info.ninputs * 32) {
    fprintf(stderr, "witness has %zu bytes, the circuit wants %zu inputs x 32\n", wit.size(), info.ninputs);
    return 2;
  }
  Set seq(B), bat(B);
  for (size_t b = 0; b < B; ++b) {
    CK(ctx, lfgpu_zk_prover_new(ctx, circ, kRate, kNreq, 0, &seq.zk[b]));
    CK(ctx, lfgpu_zk_prover_new(ctx, circ, kRate, kNreq, 0, &bat.zk[b]));
  }
  lfgpu_zk_batch256* batch = nullptr;
  CK(ctx, lfgpu_zk_batch256_new(ctx, circ, B, &batch));
  std::vector<const void*> Ws(B, wit.data());
  std::vector<int> oks(B);
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  auto commit_sequential = [&](Set& s) {
    const auto t0 = now();
    for (size_t b = 0; b < B; ++b) CK(ctx, lfgpu_zk_commit(s.zk[b], wit.data(), rng_bytes, s.rng[b], &s.ops[b], &s.roots[32 * b]));
    return ms(t0, now());
  };
  auto commit_batched = [&](Set& s) {
    const auto t0 = now();
    CK(ctx, lfgpu_zk_commit_batch256(batch, s.zk.data(), B, Ws.data(), s.fns.data(), s.users.data(), s.opsp.data(), s.roots.data()));
    return ms(t0, now());
  };
  auto prove = [&](Set& s, const char* what) {
    const auto t0 = now();
    CK(ctx, lfgpu_zk_prove_batch256(batch, s.zk.data(), B, Ws.data(), s.opsp.data(), oks.data()));
    const double t = ms(t0, now());
    for (size_t b = 0; b < B; ++b)
      if (!oks[b]) {
        fprintf(stderr, "%s: the witness does not satisfy the circuit (statement %zu)\n", what, b);
        exit(1);
      }
    return t;
  };

  // the check: sequential commits on one set, one batched commit on the other, the same seeds
  seq.reseed(0);
  bat.reseed(0);
  commit_sequential(seq);
  commit_batched(bat);
  bool roots_equal = seq.roots == bat.roots, proofs_equal = true;
  if (!roots_equal) fprintf(stderr, "the batched roots differ from lfgpu_zk_commit's\n");
  prove(seq, "after lfgpu_zk_commit");
  prove(bat, "after lfgpu_zk_commit_batch256");
  size_t proof_bytes = 0;
  std::vector<uint8_t> first;
  for (size_t b = 0; b < B; ++b) {
    const std::vector<uint8_t> want = wire_of(ctx, seq.zk[b]), got = wire_of(ctx, bat.zk[b]);
    proof_bytes = got.size();
    if (got != want) {
      fprintf(stderr, "statement %zu: the proof after the batched commit differs from the one after lfgpu_zk_commit (%zu vs %zu bytes)\n", b, got.size(), want.size());
      proofs_equal = false;
    }
    if (b == 0) first = want;
    else if (want == first) {
      fprintf(stderr, "statement %zu: same proof as statement 0 -- the seeds do not differ\n", b);
      proofs_equal = false;
    }
    const std::string tss = "ts 0 " + std::to_string(b);
    lfgpu_transcript* tv = lfgpu_transcript_new((const uint8_t*)tss.data(), tss.size());
    lfgpu_transcript_ops vops;
    lfgpu_transcript_get_ops(tv, &vops);
    int ok = 0;
    const char* why = "";
    CK(ctx, lfgpu_zk_verify(ctx, circ, kRate, kNreq, 0, got.data(), got.size(), wit.data() /*public inputs come first*/, &vops, &ok, &why));
    lfgpu_transcript_free(tv);
    if (!ok) {
      fprintf(stderr, "statement %zu: the verifier rejected the proof of the batched commit: %s\n", b, why);
      proofs_equal = false;
    }
  }

  // the bench: alternating passes on fresh seeds; the commits alone, then commit + prove_batch256
  std::vector<double> cseq, cbat, eseq, ebat;
  for (int r = 0; r < bench; ++r) {
    seq.reseed(1 + r);
    bat.reseed(1 + r);
    cseq.push_back(commit_sequential(seq) / (double)B);
    cbat.push_back(commit_batched(bat) / (double)B);
  }
  for (int r = 0; r < bench; ++r) {
    seq.reseed(1 + bench + r);
    bat.reseed(1 + bench + r);
    double t = commit_sequential(seq);
    t += prove(seq, "bench, after lfgpu_zk_commit");
    eseq.push_back(t / (double)B);
    t = commit_batched(bat);
    t += prove(bat, "bench, after lfgpu_zk_commit_batch256");
    ebat.push_back(t / (double)B);
  }
  auto med = [](std::vector<double> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
  };
  auto lo = [](const std::vector<double>& v) { return v.empty() ? 0.0 : *std::min_element(v.begin(), v.end()); };
  auto hi = [](const std::vector<double>& v) { return v.empty() ? 0.0 : *std::max_element(v.begin(), v.end()); };
  auto stat = [&](const char* key, const std::vector<double>& v, const char* end) {
    printf("\"%s\": {\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}%s", key, med(v), lo(v), hi(v), end);
  };
  printf("{\"B\": %zu, \"field\": %d, \"layers\": %zu, \"terms\": %zu, \"proof_bytes\": %zu, \"roots_equal\": %s, \"proofs_equal\": %s, \"bench_passes\": %d, ", B,
         info.field, info.nl, info.nterms, proof_bytes, roots_equal ? "true" : "false", proofs_equal ? "true" : "false", bench);
  stat("commit_sequential_ms_per_statement", cseq, ", ");
  stat("commit_batched_ms_per_statement", cbat, ", ");
  stat("pipeline_sequential_commit_ms_per_statement", eseq, ", ");
  stat("pipeline_batched_commit_ms_per_statement", ebat, "}\n");
  for (Set* s : {&seq, &bat})
    for (size_t b = 0; b < B; ++b) {
      lfgpu_transcript_free(s->ts[b]);
      lfgpu_transcript_free(s->rng[b]);
      lfgpu_zk_prover_free(s->zk[b]);
    }
  lfgpu_zk_batch256_free(batch);
  lfgpu_circuit_free(circ);
  lfgpu_shutdown(ctx);
  return roots_equal && proofs_equal ? 0 : 1;
}
