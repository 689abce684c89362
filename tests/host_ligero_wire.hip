// Host-only harness of tests/test_ligero_wire_host.py: the Ligero section of the wire format -- zkp::com_proof_read /
// com_proof_write (csrc/zk_proto.h), what lfgpu_ligero_prove emits and lfgpu_ligero_verify parses -- behind a small C ABI.
// Compiled with hipcc --cuda-host-only and linked against liblfgpu.so for the host helpers the header calls (the GF(2^128)
// constants).  With -DHLW_MAIN it is a stand-alone program (for a host sanitizer build): `prog proof.bin nw nq rateinv nreq block_enc`.
#include "../longfellow-zk_amd/csrc/zk_proto.h"

namespace {
struct Gf {  // GF(2^128): the subfield tables without a context
  GfHostCtx g;
  zkp::SubfieldSolver sub;
  explicit Gf(int k) {
    lf_gf_ctx_build(&g, k);
    sub.build(&g);
  }
};
zkp::Wire16 wire16(int field, int k) {
  zkp::Wire16 w;
  w.field = field;
  if (field == LFGPU_FIELD_GF2_128) {
    static const Gf gf4(4), gf5(5);
    const Gf& gf = k == 5 ? gf5 : gf4;
    w.g = &gf.g;
    w.sub = &gf.sub;
  }
  return w;
}
}  // namespace

extern "C" {
// com_proof_read of buf[0, len) -- the whole input must be consumed, as lfgpu_ligero_verify asks -- then com_proof_write into out.
// Returns 1 and *nbytes, *npath, and in runs[0 .. *nruns) the lengths of the alternating full-field / subfield runs of the opened
// columns (GF(2^128); a prime field has one subfield run), or 0 when the input does not parse, or -1 when out is too small.
int hlw_roundtrip(int field, int k, const lfgpu_ligero_param* p, const uint8_t* buf, size_t len, uint8_t* out, size_t cap, size_t* nbytes, size_t* npath,
                  size_t* runs, size_t cap_runs, size_t* nruns) {
  const zkp::Wire16 pol = wire16(field, k);
  zkp::ComProof<elt_t> pr;
  zkp::WireReader<zkp::Wire16> rd{pol, buf, len};
  if (!zkp::com_proof_read(rd, *p, pr) || rd.bad || rd.left != 0) return 0;
  *npath = pr.npath;
  *nruns = 0;
  if (pol.two_byte_subfield()) {
    bool sub = false;
    size_t run = 0;
    for (size_t i = 0; i < pr.req.size(); ++i) {
      const bool in_sub = zkp::Wire16::is_zero(pol.solve_subfield(pr.req[i]).first);
      while (in_sub != sub) {  // the run ends (an empty first run when the first element lies in the subfield)
        if (*nruns < cap_runs) runs[*nruns] = run;
        ++*nruns;
        run = 0;
        sub = !sub;
      }
      ++run;
    }
    if (*nruns < cap_runs) runs[*nruns] = run;
    ++*nruns;
  }
  std::vector<uint8_t> o;
  zkp::com_proof_write(pol, pr, o);
  *nbytes = o.size();
  if (o.size() > cap) return -1;
  memcpy(out, o.data(), o.size());
  return 1;
}
}  // extern "C"

#ifdef HLW_MAIN
#include <cstdio>
#include <cstdlib>
// round trip of the file's bytes, then the same input one byte short and one byte long: exit status 0 iff the first reproduces the
// input and the other two are refused
int main(int argc, char** argv) {
  if (argc != 7) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> in;
  uint8_t chunk[4096];
  for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) in.insert(in.end(), chunk, chunk + n);
  fclose(f);
  lfgpu_ligero_param p;
  if (lfgpu_ligero_param_init(&p, LFGPU_FIELD_GF2_128, 4, strtoul(argv[2], 0, 10), strtoul(argv[3], 0, 10), strtoul(argv[4], 0, 10), strtoul(argv[5], 0, 10),
                              strtoul(argv[6], 0, 10)))
    return 2;
  std::vector<uint8_t> out(in.size() + 16), longer(in);
  longer.push_back(0);
  size_t nbytes = 0, npath = 0, runs[8], nruns = 0;
  const int a = hlw_roundtrip(LFGPU_FIELD_GF2_128, 4, &p, in.data(), in.size(), out.data(), out.size(), &nbytes, &npath, runs, 8, &nruns);
  const bool same = a == 1 && nbytes == in.size() && memcmp(out.data(), in.data(), nbytes) == 0;
  const int b = hlw_roundtrip(LFGPU_FIELD_GF2_128, 4, &p, in.data(), in.size() - 1, out.data(), out.size(), &nbytes, &npath, runs, 8, &nruns);
  const int c = hlw_roundtrip(LFGPU_FIELD_GF2_128, 4, &p, longer.data(), longer.size(), out.data(), out.size(), &nbytes, &npath, runs, 8, &nruns);
  printf("round trip %s, truncated %s, over-long %s\n", same ? "same bytes" : "DIFFERS", b == 0 ? "refused" : "ACCEPTED", c == 0 ? "refused" : "ACCEPTED");
  return same && b == 0 && c == 0 ? 0 : 1;
}
#endif
