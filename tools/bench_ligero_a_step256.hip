// bench_ligero_a_step256.hip -- the A step of the Ligero dot proof over Fp256Base alone, two routes in one process
// (profiles/ligero_prove_p256/README.md):
//   device: the 48-byte term records as they stand -> lf_lig256_a_rows_terms (a_terms256_kernel: wave fold + limb atomics, csrc/zk256.hip)
//   host:   zkp::inner_product_sparse (multiply, sort, fold on the host) -> lf_lig256_a_rows_sparse (a_rows_sparse256_kernel)
// on LigeroParam(nw 700, nq 40, rateinv 4, nreq 12, block_enc 512) with random terms over nl = 64 constraints and all 700 wires.
// 7 alternating passes after one warm-up, median and range of the wall time including the final synchronise; the two routes'
// rows are compared.
//   hipcc -O2 -std=c++17 tools/bench_ligero_a_step256.hip -Llongfellow-zk_amd -l:liblfgpu.so -Wl,-rpath,'$ORIGIN/../longfellow-zk_amd' -o tools/bench_ligero_a_step256
#include <algorithm>
#include <cstdio>
#include <random>

#include "../longfellow-zk_amd/csrc/zk_proto.h"

#define CK(x)                                                     \
  do {                                                            \
    int rc_ = (x);                                                \
    if (rc_) {                                                    \
      fprintf(stderr, "%s failed (%d) at line %d\n", #x, rc_, __LINE__); \
      return 1;                                                   \
    }                                                             \
  } while (0)

int main(int argc, char** argv) {
  const size_t nterm = argc > 1 ? strtoul(argv[1], 0, 10) : (size_t)1 << 20, nl = 64;
  lfgpu_ctx* c = nullptr;
  CK(lfgpu_init(0, &c));
  lfgpu_ligero_param p;
  CK(lfgpu_ligero_param_init(&p, LFGPU_FIELD_P256, 0, 700, 40, 4, 12, 512));
  printf("shape: nrow %zu, nwqrow %zu, w %zu, block_enc %zu; %zu terms over %zu wires, nl %zu\n", p.nrow, p.nwqrow, p.w, p.block_enc, nterm, p.nw, nl);
  std::mt19937_64 rng(7);
  auto elt = [&] {  // a uniform element: the Montgomery image of a value below p
    for (;;) {
      elt32_t e{{rng(), rng(), rng(), rng()}};
      if (h256_fits(e)) return e;
    }
  };
  std::vector<lfgpu_ligero_llterm256> ll(nterm);
  std::vector<zkp::LinTerm<elt32_t>> lin(nterm);
  for (size_t t = 0; t < nterm; ++t) {
    const elt32_t k = elt();
    ll[t] = {rng() % nl, rng() % p.nw, {k.l[0], k.l[1], k.l[2], k.l[3]}};
    lin[t] = {ll[t].c, ll[t].w, k};
  }
  std::vector<elt32_t> alphal(nl), alphaq(3 * p.nq);
  for (auto& e : alphal) e = elt();
  for (auto& e : alphaq) e = elt();
  std::vector<size_t> lqc(3 * p.nq);
  for (auto& x : lqc) x = rng() % p.nw;
  const size_t ld = p.dblock, nelt = p.nwqrow * ld;
  void* d_rows = nullptr;
  CK(lfgpu_malloc(c, nelt * 32, &d_rows));
  const F256 F;
  std::vector<elt32_t> got[2] = {std::vector<elt32_t>(nelt), std::vector<elt32_t>(nelt)};
  std::vector<double> ms[2];
  for (int pass = 0; pass < 8; ++pass)  // pass 0 warms both routes up (scratch growth, code load)
    for (int route = 0; route < 2; ++route) {
      CK(hipMemset(d_rows, 0, nelt * 32) != hipSuccess);
      CK(lfgpu_sync(c));
      const double t0 = zkp::now_ms();
      if (route == 0) {
        CK(lf_lig256_a_rows_terms(c, &p, ld, ll.data(), nterm, alphal.data(), nl, lqc.data(), alphaq.data(), d_rows));
      } else {
        std::vector<uint64_t> idx;
        std::vector<elt32_t> val;
        zkp::inner_product_sparse<zkp::Wire32>(F, p, lin, alphal, lqc, alphaq, idx, val);
        CK(lf_lig256_a_rows_sparse(c, &p, ld, idx.data(), val.data(), idx.size(), d_rows));
      }
      CK(lfgpu_sync(c));
      if (pass) ms[route].push_back(zkp::now_ms() - t0);
      CK(lfgpu_memcpy_d2h(c, got[route].data(), d_rows, nelt * 32));
    }
  const bool same = memcmp(got[0].data(), got[1].data(), nelt * 32) == 0;
  for (int route = 0; route < 2; ++route) {
    std::sort(ms[route].begin(), ms[route].end());
    printf("%-6s median %.3f ms (min %.3f, max %.3f) over %zu passes\n", route ? "host" : "device", ms[route][ms[route].size() / 2], ms[route].front(),
           ms[route].back(), ms[route].size());
  }
  printf("rows of the two routes: %s\n", same ? "identical" : "DIFFER");
  lfgpu_free(c, d_rows);
  lfgpu_shutdown(c);
  return same ? 0 : 1;
}
