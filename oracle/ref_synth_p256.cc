// ref_synth_p256.cc -- SYNTHETIC ZK fixtures over Fp256Base from the real reference (build container only).  The two fixed
// P-256 circuits (the mdoc signature circuit, the 2-layer "sgonal" toy of ref_small_p256.cc) leave most of the shape
// space of csrc/zk256.hip untouched; this program builds layered arithmetic circuits from a short seeded description
// with the reference's own compiler (QuadCircuit + CompilerBackend + Logic, mkcircuit(1)), proves them with
// ZkProver<Field, .> under the fixtures' transcript ("test") and LCG RandomEngine, checks the proof with the
// reference's ZkVerifier and records what a test needs to pin the library on the same bytes.
//
//   gen_synth_p256 <case> <outdir>   ->  <outdir>/synth_p256_<case>.lfc1  CircuitWriter bytes
//                                        <outdir>/synth_p256_<case>.w     witness, ninputs x 32-byte in-memory Elt images
//                                        <outdir>/synth_p256_<case>.json  shapes as compiled, LigeroParam, SHA-256 of the
//                                                                         proof and of every section of ZkProof::write
//   gen_synth_p256 --list            ->  the case names
// oracle/gen_synth_p256_fixtures.py compresses the two binary files and collects the records in tests/golden/synth_p256.json.
//
// ref_synth_fp128.cc compiles this same text over Fp128 (REF_SYNTH_FP128: 16-byte elements, the file stem synth_fp128_, the
// FFT Reed-Solomon factory of ref_flatsha.cc under REF_FP128, a case table of its own) into gen_synth_fp128, and
// ref_synth_gf.cc over GF2_128<> (REF_SYNTH_GF2_128: the stem synth_gf_, the LCH14 Reed-Solomon factory of ref_flatsha.cc, a
// case table of its own) into gen_synth_gf.  What differs in characteristic 2 stands under "GF(2^128)" below.
//
// A layer of B gates over the A wires below it: gate j is a sum of T products P[a] * P[b], the pairs taken in order from
// pair(m) = (2m mod A, 2m + 1 + 2 floor(2m / A) mod A), m = jT .. jT + T - 1, T >= ceil(A / 2B) so that every wire below is
// read.  "hub" adds the product hub * P[j mod A] to every gate (one wire read by every gate), "common" adds the same product
// P[0] * P[2] to every gate (one hand pair shared by every gate).  The last layer's gates are the outputs: the program
// evaluates every gate in the field as it builds it, feeds each output's value in as one more input and asserts
// gate - input == 0, so the circuit is satisfied by construction.  The only constants are 1 and -1; input values come from a
// pool of 61 LCG-drawn elements, with 0, 1 and p - 1 on the data inputs 1, 2, 3.
//
// GF(2^128).  LigeroProver::commit refuses a witness below subfield_boundary that is not in the 16-bit subfield, so in a case
// that calls begin_full_field() every data input created before the call comes from a second pool of 61 values drawn with
// RandomEngine::subfield_elt; the inputs after it come from the full-field pool.  -1 == 1, so the data input 3 holds
// of_scalar(0xffff), the element whose subfield coordinates are all ones (legal on either side of the boundary; the record
// names it input_ones).  1 + 1 == 0: a product that occurs twice in one gate vanishes from the compiled circuit.  The
// descriptions of the table avoid that (pair(m) repeats only after A^2 / 4 pairs; the hub and common products never
// equal a pair product of their gate at these sizes), and tests/test_zk_gf_synth.py recounts terms, hand pairs, fan-in and
// fan-out from the LFC1 bytes.  The record also holds the run structure of the opened columns, parsed from the wire bytes
// (run lengths, number of 16-byte and of 2-byte elements) and subfield_boundary - npub_in, the boundary LigeroProver gets.
// CPU time of the whole table: 14 s, 13 of them in wide (compile and prove of two layers of 263006 wires).
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "algebra/convolution.h"
#include "algebra/fp2.h"
#include "algebra/fp_p128.h"
#include "algebra/reed_solomon.h"
#include "arrays/dense.h"
#include "circuits/compiler/compiler.h"
#include "circuits/logic/compiler_backend.h"
#include "circuits/logic/logic.h"
#include "ec/p256.h"
#include "gf2k/gf2_128.h"
#include "gf2k/lch14_reed_solomon.h"
#include "proto/circuit_io.h"
#include "proto/circuit_writer.h"
#include "random/random.h"
#include "random/transcript.h"
#include "sumcheck/circuit.h"
#include "sumcheck/quad_builder.h"
#include "util/crypto.h"
#include "util/log.h"
#include "zk/zk_proof.h"
#include "zk/zk_prover.h"
#include "zk/zk_verifier.h"

using namespace proofs;

class LcgRng : public RandomEngine {
 public:
  explicit LcgRng(uint64_t seed) : s_(seed) {}
  void bytes(uint8_t* buf, size_t n) override {
    for (size_t i = 0; i < n; ++i) {
      s_ = s_ * 6364136223846793005ull + 1442695040888963407ull;
      buf[i] = static_cast<uint8_t>(s_ >> 32);
    }
  }

 private:
  uint64_t s_;
};

#if defined(REF_SYNTH_GF2_128)
using Field = GF2_128<>;
static const Field kField;
static const FieldID kFieldId = GF2_128_ID;
#define SYNTH_STEM "synth_gf_"
#define SYNTH_THIRD_KEY "input_ones"
// the LCH14 Reed-Solomon factory as ref_flatsha.cc sets it up for GF(2^128)
using RSFactory_b = LCH14ReedSolomonFactory<Field>;
struct RSSetup {
  const RSFactory_b rsf;
  explicit RSSetup(const Field& F) : rsf(F) {}
};
#elif defined(REF_SYNTH_FP128)
using Field = Fp128<>;
static const Field kField;
static const FieldID kFieldId = FP128_ID;
#define SYNTH_STEM "synth_fp128_"
#define SYNTH_THIRD_KEY "input_mone"
// the FFT Reed-Solomon factory as lib/zk/zk_test.cc sets it up for Fp128 (ref_flatsha.cc under REF_FP128)
using FftConv = FFTConvolutionFactory<Field>;
using RSFactory_b = ReedSolomonFactory<Field, FftConv>;
struct RSSetup {
  const FftConv fft;
  const RSFactory_b rsf;
  explicit RSSetup(const Field& F) : fft(F, F.of_string("164956748514267535023998284330560247862"), 1ull << 32), rsf(fft, F) {}
};
#else
using Field = Fp256Base;
static const Field& kField = p256_base;
static const FieldID kFieldId = P256_ID;
#define SYNTH_STEM "synth_p256_"
#define SYNTH_THIRD_KEY "input_mone"
using f2_p256 = Fp2<Fp256Base>;
using FftExtConvolutionFactory = FFTExtConvolutionFactory<Fp256Base, f2_p256>;
using RSFactory_b = ReedSolomonFactory<Fp256Base, FftExtConvolutionFactory>;
struct RSSetup {
  const f2_p256 p256_2;
  const FftExtConvolutionFactory fft;
  const RSFactory_b rsf;
  // the root of unity of order 2^31 in the quadratic extension (lib/circuits/mdoc/mdoc_zk.cc:82-88)
  explicit RSSetup(const Field& F)
      : p256_2(F),
        fft(F, p256_2,
            p256_2.of_string("112649224146410281873500457609690258373018840430489408729223714171582664680802",
                             "84087994358540907695740461427818660560182168997182378749313018254450460212908"),
            1ull << 31),
        rsf(fft, F) {}
};
#endif
constexpr size_t kEltBytes = sizeof(Field::Elt);  // the in-memory image is the wire size in both fields

struct LayerSpec {
  size_t gates;  // gates of this layer (the copy wires of wire 0 and of the outputs' values come on top)
  size_t tmin;   // least number of pair products per gate
  bool hub;      // + hub * P[j mod A] in gate j
  bool common;   // + P[0] * P[2] in every gate
};
struct CaseSpec {
  const char* name;
  uint64_t seed;  // of the value pool; the prover's RandomEngine is LcgRng(100) as in every fixture
  size_t rate, nreq, block_enc;  // block_enc 0: LigeroParam's own search
  size_t npub;       // public data inputs (wire 0 comes on top)
  bool pub_outputs;  // the outputs' values are public inputs (else the last private ones)
  size_t nsub;       // private data inputs before begin_full_field() (0: never called)
  size_t npriv;      // private data inputs in all
  std::vector<LayerSpec> layers;  // from the inputs up; the last one's gates are the outputs
};

static const std::vector<CaseSpec>& cases() {
  static const std::vector<CaseSpec> c = {
#if defined(REF_SYNTH_GF2_128)
      // wide: as over Fp128 -- two layers beyond 2^18 wires and beyond 262144 hand pairs, a wire read by every gate of such a
      // layer and (here) one hand pair in every gate of it, gates of more than 1024 terms; rate 5, 40 queries, block_enc by
      // the reference's search
      {"wide", 31, 5, 40, 0, 0, false, 0, 2000, {{263000, 2, false, false}, {263000, 1, true, true}, {30, 4384, false, false}, {5, 3, false, false}}},
      // odd: 2^12 + 1 inputs, then 3 * 2^10, 5000 and 2^10 + 1 wires; begin_full_field() after exactly three witness
      // rows of the recorded LigeroParam (w = 323, which does not depend on where the boundary lies): the last subfield-only
      // row ends ON the boundary, and the input right after it holds a full-field pool value
      {"odd", 32, 7, 132, 0, 0, false, 3 * 323, 4093, {{3068, 1, false, false}, {4996, 1, false, true}, {1021, 3, false, false}, {100, 6, false, false}, {3, 17, false, false}}},
      // funnel: 9 down to 2 output variables and 0; rate 4 and 6 queries, so that the search settles on a small block_enc
      // (block <= 128: LCH14 plans of fewer than 7 levels)
      {"funnel", 33, 4, 6, 0, 0, false, 0, 300, {{398, 1, false, false}, {198, 1, false, false}, {98, 1, false, false}, {48, 1, false, false}, {22, 1, false, false},
                                                  {10, 1, false, false}, {4, 1, false, false}, {2, 1, false, false}, {1, 1, false, false}}},
      // tall: block_enc 24581 at rate 4 is the least with block > 4096 (4097; dblock 8193): every row takes the general
      // encoder, and 120000 private inputs make 30 witness rows, so that the rows after IQUAD -- one call of 33 rows -- take
      // its bit-sliced tower variant.  Public inputs (data and outputs); begin_full_field() 9000 inputs in: two
      // subfield-only rows, a mixed one, full rows
      {"tall", 34, 4, 30, 24581, 5, true, 9000, 120000, {{2000, 10, false, false}, {100, 10, false, false}, {4, 13, false, false}}},
      // long: a small circuit in the widest tableau the field admits (evaluation points must exist in the 16-bit subfield):
      // 7 rows through the plain variant of the general encoder, the last LCH14 coset partial for block and for dblock; two
      // outputs (one output variable)
      {"long", 35, 4, 20, 65535, 0, false, 0, 3000, {{500, 3, false, false}, {40, 7, false, false}, {2, 10, false, false}}},
#elif defined(REF_SYNTH_FP128)
      // wide: two layers beyond 2^18 wires and beyond 262144 hand pairs (two round-hands on the per-launch kernels before the
      // resident grid's hand-off point of 131072), a wire read by every gate of such a layer, gates of more than 1024 terms;
      // rate and query count other than the flatsha fixture's (7, 132), block_enc by the reference's search
      {"wide", 21, 5, 40, 0, 0, false, 0, 2000, {{263000, 2, false, false}, {263000, 1, true, false}, {30, 4384, false, false}, {5, 3, false, false}}},
      // odd: as over Fp256Base -- 2^12 + 1 inputs, then 3 * 2^10, 5000 and 2^10 + 1 wires; one hand pair in every gate of the 5000
      {"odd", 22, 7, 132, 0, 0, false, 0, 4093, {{3068, 1, false, false}, {4996, 1, false, true}, {1021, 3, false, false}, {100, 6, false, false}, {3, 17, false, false}}},
      // funnel: 9 down to 2 output variables and 0 (one output), layers that start within one wave (<= 64 wires), ending in
      // layers of 6 wires and 4 hand pairs, 4 wires and 2
      {"funnel", 23, 4, 6, 0, 0, false, 0, 300, {{398, 1, false, false}, {198, 1, false, false}, {98, 1, false, false}, {48, 1, false, false}, {22, 1, false, false},
                                                  {10, 1, false, false}, {4, 1, false, false}, {2, 1, false, false}, {1, 1, false, false}}},
      // tall: 40000 inputs in a tableau of 16384 columns (the two-pass FFT plan), public inputs (data and outputs);
      // begin_full_field() several witness rows in, which only the header shows in this field
      {"tall", 24, 4, 30, 16384, 5, true, 9000, 40000, {{2000, 10, false, false}, {100, 10, false, false}, {4, 13, false, false}}},
      // long: a small circuit in a tableau of 2^18 columns, so that the commitment's RS encode runs the FFT at 2^18 points
      // (at 2^20 the reference takes 17 s and the GPU test 9.5 s; 2^18 keeps both within a few seconds);
      // two outputs (one output variable: the layer under a single output has wire 0, the output's input and a gate, so
      // the funnel cannot hold it)
      {"long", 25, 4, 20, 1 << 18, 0, false, 0, 3000, {{500, 3, false, false}, {40, 7, false, false}, {2, 10, false, false}}},
#else
      // wide: layers beyond 2^16 wires and beyond 131072 hand pairs, a wire read by every gate of such a layer, gates of more
      // than 1024 terms; rate and query count of neither fixed fixture, block_enc by the reference's search
      {"wide", 11, 5, 40, 0, 0, false, 0, 1000, {{70000, 2, false, false}, {70000, 1, true, false}, {30, 1167, false, false}, {5, 3, false, false}}},
      // odd: 2^12 + 1 inputs, then 3 * 2^10, 5000 (odd after three halvings) and 2^10 + 1 wires, all above the default hand-off
      // point of the resident grid or across it; one hand pair in every gate of the 5000
      {"odd", 12, 7, 132, 0, 0, false, 0, 4093, {{3068, 1, false, false}, {4996, 1, false, true}, {1021, 3, false, false}, {100, 6, false, false}, {3, 17, false, false}}},
      // funnel: every number of output variables from 9 down to 1, ending in a layer of 6 wires and 4 hand pairs
      {"funnel", 13, 4, 6, 0, 0, false, 0, 300, {{398, 1, false, false}, {198, 1, false, false}, {98, 1, false, false}, {48, 1, false, false}, {22, 1, false, false},
                                                  {10, 1, false, false}, {4, 1, false, false}, {2, 1, false, false}, {1, 1, false, false}}},
      // tall: 40000 inputs in a tableau of 16384 columns, public inputs, a subfield boundary several witness rows in
      {"tall", 14, 4, 30, 16384, 5, true, 9000, 40000, {{2000, 10, false, false}, {100, 10, false, false}, {4, 13, false, false}}},
#endif
  };
  return c;
}

static std::string hexs(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}
static std::string sha_hex(const uint8_t* p, size_t n) {
  uint8_t dg[32];
  proofs::SHA256 sha;
  sha.Update(p, n);
  sha.DigestData(dg);
  return hexs(dg, 32);
}
static bool write_file(const std::string& path, const void* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(p, 1, n, f) == n;
  return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
  set_log_level(ERROR);
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const auto& c : cases()) printf("%s\n", c.name);
    return 0;
  }
  if (argc != 3) {
    fprintf(stderr, "usage: %s <case> <outdir> | --list\n", argv[0]);
    return 2;
  }
  const CaseSpec* cs = nullptr;
  for (const auto& c : cases())
    if (!strcmp(c.name, argv[1])) cs = &c;
  if (!cs) {
    fprintf(stderr, "unknown case %s\n", argv[1]);
    return 2;
  }
  using Backend = CompilerBackend<Field>;
  using LogicCircuit = Logic<Field, Backend>;
  using EltW = LogicCircuit::EltW;
  using Elt = Field::Elt;
  const Field& F = kField;

  // the value pool(s)
  Elt pool[61];
  {
    LcgRng vr(cs->seed);
    for (auto& e : pool) e = vr.elt(F);
  }
#ifdef REF_SYNTH_GF2_128
  Elt subpool[61];
  {
    LcgRng vr(cs->seed + 1000);
    for (auto& e : subpool) e = vr.subfield_elt(F);
  }
  bool full_field = cs->nsub == 0;  // no begin_full_field(): subfield_boundary stays 0 and nothing is promised
#endif
  const size_t nout = cs->layers.back().gates;
  std::vector<Elt> wit;  // by input index
  std::vector<size_t> out_input(nout);
  std::unique_ptr<Circuit<Field>> circuit;
  size_t special[3] = {0, 0, 0};
  {
    QuadCircuit<Field> Q(F);
    Backend cbk(&Q);
    const LogicCircuit LC(&cbk, F);
    wit.push_back(F.one());  // wire 0
    std::vector<EltW> P;     // the data wires of the layer below, and their values
    std::vector<Elt> PV;
    std::vector<EltW> outs(nout);
    auto data_input = [&]() {
      const size_t i = P.size();
      Elt v = pool[(i * 7 + i / 61) % 61];
#ifdef REF_SYNTH_GF2_128
      if (!full_field) v = subpool[(i * 7 + i / 61) % 61];
      const Elt third = F.of_scalar(0xffff);
#else
      const Elt third = F.mone();
#endif
      if (i == 1) v = F.zero();
      if (i == 2) v = F.one();
      if (i == 3) v = third;
      if (i >= 1 && i <= 3) special[i - 1] = wit.size();
      P.push_back(LC.eltw_input());
      PV.push_back(v);
      wit.push_back(v);
    };
    auto out_inputs = [&]() {
      for (size_t k = 0; k < nout; ++k) {
        out_input[k] = wit.size();
        outs[k] = LC.eltw_input();
        wit.push_back(F.zero());  // set below
      }
    };
    for (size_t i = 0; i < cs->npub; ++i) data_input();
    if (cs->pub_outputs) out_inputs();
    Q.private_input();
    for (size_t i = 0; i < cs->npriv; ++i) {
      if (cs->nsub && i == cs->nsub) {
        Q.begin_full_field();
#ifdef REF_SYNTH_GF2_128
        full_field = true;
#endif
      }
      data_input();
    }
    if (!cs->pub_outputs) out_inputs();

    for (const LayerSpec& ls : cs->layers) {
      const size_t A = P.size(), B = ls.gates;
      const size_t T = std::max(ls.tmin, (A + 2 * B - 1) / (2 * B));
      std::vector<EltW> N;
      std::vector<Elt> NV;
      for (size_t j = 0; j < B; ++j) {
        const size_t m0 = j * T, a0 = (2 * m0) % A, b0 = (a0 + 1 + 2 * ((2 * m0) / A)) % A;
        EltW g = LC.mul(P[a0], P[b0]);
        Elt v = F.mulf(PV[a0], PV[b0]);
        for (size_t t = 1; t < T; ++t) {
          const size_t m = m0 + t, a = (2 * m) % A, b = (a + 1 + 2 * ((2 * m) / A)) % A;
          g = LC.add(g, LC.mul(P[a], P[b]));
          F.add(v, F.mulf(PV[a], PV[b]));
        }
        if (ls.hub) {
          g = LC.add(g, LC.mul(P[3], P[j % A]));
          F.add(v, F.mulf(PV[3], PV[j % A]));
        }
        if (ls.common) {
          g = LC.add(g, LC.mul(P[0], P[2]));
          F.add(v, F.mulf(PV[0], PV[2]));
        }
        N.push_back(g);
        NV.push_back(v);
      }
      P.swap(N);
      PV.swap(NV);
    }
    for (size_t k = 0; k < nout; ++k) {
      wit[out_input[k]] = PV[k];
      LC.assert0(LC.sub(P[k], outs[k]));
    }
    circuit = Q.mkcircuit(1);
  }
  const Circuit<Field>& c = *circuit;
  if (wit.size() != c.ninputs) return 3;

  std::vector<uint8_t> cb;
  CircuitWriter<Field> cw(F, kFieldId);
  cw.to_bytes(c, cb);
  auto W = Dense<Field>(1, c.ninputs);
  for (size_t i = 0; i < c.ninputs; ++i) W.v_[i] = wit[i];

  const RSSetup rs(F);
  const RSFactory_b& rsf = rs.rsf;
  auto mkproof = [&]() { return cs->block_enc ? ZkProof<Field>(c, cs->rate, cs->nreq, cs->block_enc) : ZkProof<Field>(c, cs->rate, cs->nreq); };
  ZkProof<Field> zk = mkproof();
  ZkProver<Field, RSFactory_b> zp(c, F, rsf);
  Transcript tp((const uint8_t*)"test", 4);
  LcgRng rng(100);
  zp.commit(zk, W, tp, rng);
  if (!zp.prove(zk, W, tp)) return 4;
  std::vector<uint8_t> wire;
  zk.write(wire, F);

  // the reference's verifier on the bytes as a verifier gets them
  bool vok = false;
  {
    ZkProof<Field> zr = mkproof();
    ReadBuffer rb(wire);
    if (!zr.read(rb, F) || rb.remaining() != 0) return 6;
    std::unique_ptr<ZkVerifier<Field, RSFactory_b>> zv;
    if (cs->block_enc)
      zv = std::make_unique<ZkVerifier<Field, RSFactory_b>>(c, rsf, cs->rate, cs->nreq, cs->block_enc, F);
    else
      zv = std::make_unique<ZkVerifier<Field, RSFactory_b>>(c, rsf, cs->rate, cs->nreq, F);
    Transcript tv((const uint8_t*)"test", 4);
    zv->recv_commitment(zr, tv);
    auto pub = Dense<Field>(1, c.npub_in);
    for (size_t i = 0; i < c.npub_in; ++i) pub.v_[i] = W.v_[i];
    vok = zv->verify(zr, pub, tv);
  }

  // the record
  const std::string stem = std::string(argv[2]) + "/" SYNTH_STEM + cs->name;
  if (!write_file(stem + ".lfc1", cb.data(), cb.size()) || !write_file(stem + ".w", W.v_.data(), kEltBytes * c.ninputs)) return 7;
  FILE* js = fopen((stem + ".json").c_str(), "w");
  if (!js) return 7;
  const auto& p = zk.param;
  fprintf(js, "{\"case\": \"%s\", \"nl\": %zu, \"ninputs\": %zu, \"npub_in\": %zu, \"nv\": %zu, \"logv\": %zu, \"subfield_boundary\": %zu, \"nterms\": %zu, \"nconst\": ", cs->name,
          c.nl, c.ninputs, c.npub_in, (size_t)c.nv, c.logv, c.subfield_boundary, c.nterms());
  {
    KvecBuilder<Field> kb(F);
    for (const auto& layer : c.l)
      for (const auto& ec : *layer.quad) kb.kstore(ec.v);
    fprintf(js, "%zu, ", kb.kvec()->size());
  }
  fprintf(js, "\"lfc1_bytes\": %zu, \"lfc1_sha256\": \"%s\", \"witness_sha256\": \"%s\", ", cb.size(), sha_hex(cb.data(), cb.size()).c_str(),
          sha_hex((const uint8_t*)W.v_.data(), kEltBytes * c.ninputs).c_str());
  fprintf(js, "\"input_zero\": %zu, \"input_one\": %zu, \"" SYNTH_THIRD_KEY "\": %zu, \"first_output_input\": %zu, \"noutput_inputs\": %zu, ", special[0], special[1], special[2],
          out_input[0], nout);
  fprintf(js, "\"layers\": [");
  for (size_t i = 0; i < c.nl; ++i) {
    const size_t lnv = i == 0 ? (size_t)c.nv : (size_t)c.l[i - 1].nw, llogv = i == 0 ? c.logv : c.l[i - 1].logw;
    std::map<std::pair<size_t, size_t>, size_t> pairs;
    std::map<size_t, size_t> gate, reads;
    for (const auto& ec : *c.l[i].quad) {
      const size_t h0 = (size_t)ec.h[0], h1 = (size_t)ec.h[1];
      ++pairs[{h0, h1}];
      ++gate[(size_t)ec.g];
      ++reads[h0];
      if (h1 != h0) ++reads[h1];
    }
    size_t mp = 0, mg = 0, mr = 0;
    for (const auto& kv : pairs) mp = std::max(mp, kv.second);
    for (const auto& kv : gate) mg = std::max(mg, kv.second);
    for (const auto& kv : reads) mr = std::max(mr, kv.second);
    fprintf(js, "%s{\"logv\": %zu, \"nv\": %zu, \"logw\": %zu, \"nw\": %zu, \"nterms\": %zu, \"nh0\": %zu, \"max_gate_terms\": %zu, \"max_pair_terms\": %zu, \"max_wire_reads\": %zu}",
            i ? ", " : "", llogv, lnv, c.l[i].logw, (size_t)c.l[i].nw, c.l[i].nterms(), pairs.size(), mg, mp, mr);
  }
  fprintf(js, "], \"rate\": %zu, \"nreq\": %zu, \"block_enc_arg\": %zu, \"pool_seed\": %llu, \"rng_seed\": 100, ", cs->rate, cs->nreq, cs->block_enc, (unsigned long long)cs->seed);
  fprintf(js,
          "\"ligero_param\": {\"nw\": %zu, \"nq\": %zu, \"rateinv\": %zu, \"nreq\": %zu, \"block_enc\": %zu, \"block\": %zu, \"dblock\": %zu, \"block_ext\": %zu, \"r\": %zu, \"w\": %zu, "
          "\"nwrow\": %zu, \"nqtriples\": %zu, \"nwqrow\": %zu, \"nrow\": %zu, \"mc_pathlen\": %zu, \"ildt\": %zu, \"idot\": %zu, \"iquad\": %zu, \"iw\": %zu, \"iq\": %zu}, ",
          p.nw, p.nq, p.rateinv, p.nreq, p.block_enc, p.block, p.dblock, p.block_ext, p.r, p.w, p.nwrow, p.nqtriples, p.nwqrow, p.nrow, p.mc_pathlen, p.ildt, p.idot, p.iquad, p.iw, p.iq);
  // the sections of ZkProof::write (lib/zk/zk_proof.h:90-184), in wire order
  const size_t npath = zk.com_proof.merkle.path.size();
  std::vector<std::pair<std::string, size_t>> sec;
  sec.push_back({"root", 32});
  for (size_t i = 0; i < c.nl; ++i) sec.push_back({"sumcheck_layer_" + std::to_string(i), (4 * c.l[i].logw + 2) * kEltBytes});
  sec.push_back({"y_ldt", p.block * kEltBytes});
  sec.push_back({"y_dot", p.dblock * kEltBytes});
  sec.push_back({"y_quad_0", p.r * kEltBytes});
  sec.push_back({"y_quad_2", (p.dblock - p.block) * kEltBytes});
  sec.push_back({"nonces", p.nreq * 32});
  size_t fixed = 4 + 32 * npath;
  for (const auto& s : sec) fixed += s.second;
  if (fixed > wire.size()) return 8;
  sec.push_back({"opened_columns", wire.size() - fixed});  // run lengths + elements
  sec.push_back({"merkle_path", 4 + 32 * npath});
  fprintf(js, "\"zk_root\": \"%s\", \"zk_wire_bytes\": %zu, \"zk_wire_sha256\": \"%s\", \"sections\": [", hexs(zk.com.root.data, 32).c_str(), wire.size(),
          sha_hex(wire.data(), wire.size()).c_str());
  size_t off = 0;
  for (size_t i = 0; i < sec.size(); ++i) {
    fprintf(js, "%s{\"name\": \"%s\", \"offset\": %zu, \"bytes\": %zu, \"sha256\": \"%s\"", i ? ", " : "", sec[i].first.c_str(), off, sec[i].second,
            sha_hex(wire.data() + off, sec[i].second).c_str());
#ifdef REF_SYNTH_GF2_128
    if (sec[i].first == "opened_columns") {
      // the run structure of ZkProof::write (zk_proof.h:156-178), read back from the wire bytes: 4-byte run lengths in front
      // of alternating runs of 16-byte and 2-byte elements, the first run full-field
      std::vector<size_t> runs;
      size_t at = off, left = p.nreq * p.nrow, nelt[2] = {0, 0};
      const size_t end = off + sec[i].second;
      while (left) {
        if (at + 4 > end) return 9;
        const size_t n = (size_t)wire[at] | (size_t)wire[at + 1] << 8 | (size_t)wire[at + 2] << 16 | (size_t)wire[at + 3] << 24;
        const bool sub = runs.size() & 1;
        at += 4 + n * (sub ? Field::kSubFieldBytes : Field::kBytes);
        if (n > left || at > end) return 9;
        nelt[sub] += n;
        left -= n;
        runs.push_back(n);
      }
      if (at != end) return 9;
      fprintf(js, ", \"runs\": [");
      for (size_t k = 0; k < runs.size(); ++k) fprintf(js, "%s%zu", k ? ", " : "", runs[k]);
      fprintf(js, "], \"full\": %zu, \"sub\": %zu", nelt[0], nelt[1]);
    }
#endif
    fprintf(js, "}");
    off += sec[i].second;
  }
  if (off != wire.size()) return 8;
  fprintf(js, "], ");
#ifdef REF_SYNTH_GF2_128
  fprintf(js, "\"ligero_subfield_boundary\": %zu, ", c.subfield_boundary >= c.npub_in ? c.subfield_boundary - c.npub_in : 0);  // zk_prover.h:83-88
#endif
  fprintf(js, "\"reference_verifier_accepts\": %s}\n", vok ? "true" : "false");
  if (fclose(js) != 0) return 7;

  // the shapes as compiled, for tuning the descriptions
  printf("%s: nl %zu ninputs %zu npub_in %zu subfield_boundary %zu nterms %zu lfc1 %zu bytes | ligero block_enc %zu nrow %zu block %zu | wire %zu bytes | verifier %s\n", cs->name, c.nl,
         c.ninputs, c.npub_in, c.subfield_boundary, c.nterms(), cb.size(), p.block_enc, p.nrow, p.block, wire.size(), vok ? "accepts" : "REJECTS");
  for (size_t i = 0; i < c.nl; ++i)
    printf("  layer %zu: nv %zu logw %zu nw %zu nterms %zu\n", i, i == 0 ? (size_t)c.nv : (size_t)c.l[i - 1].nw, c.l[i].logw, (size_t)c.l[i].nw, c.l[i].nterms());
  return vok ? 0 : 5;
}
