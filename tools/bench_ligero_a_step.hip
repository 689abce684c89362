// bench_ligero_a_step.hip -- the A step of the Ligero dot proof alone, two routes in one process (profiles/ligero_prove/README.md):
//   device: the term list as it stands -> lf_ligero_a_rows_terms (atomic accumulation, csrc/ligero.hip)
//   host:   zkp::inner_product_sparse (multiply, sort, fold on the host) -> lfgpu_ligero_inner_product_rows (a_rows_sparse)
// on the flatsha-32 Ligero shape (GF2_128, nw 111760, nq 1: 150 rows, block_enc 8192) with a synthetic list of 2^20 terms over
// about 10^5 distinct wires.  7 alternating passes, median and range of the wall time including the final synchronise; the two
// routes' rows are compared.
//   hipcc -O2 -std=c++17 tools/bench_ligero_a_step.hip -Llongfellow-zk_amd -l:liblfgpu.so -Wl,-rpath,'$ORIGIN/../longfellow-zk_amd' -o tools/bench_ligero_a_step
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
  const size_t nterm = argc > 1 ? strtoul(argv[1], 0, 10) : (size_t)1 << 20, ndistinct = argc > 2 ? strtoul(argv[2], 0, 10) : 100000, nl = 1024;
  lfgpu_ctx* c = nullptr;
  CK(lfgpu_init(0, &c));
  const int field = LFGPU_FIELD_GF2_128;
  lfgpu_ligero_param p;
  CK(lfgpu_ligero_param_init(&p, field, 4, 111760, 1, 7, 132, 8192));
  printf("shape: nrow %zu, nwqrow %zu, w %zu, block_enc %zu; %zu terms over %zu wires, nl %zu\n", p.nrow, p.nwqrow, p.w, p.block_enc, nterm, ndistinct, nl);
  std::mt19937_64 rng(7);
  std::vector<size_t> wires(ndistinct);
  for (auto& w : wires) w = rng() % p.nw;
  std::vector<lfgpu_ligero_llterm> ll(nterm);
  std::vector<zkp::LinTerm<elt_t>> lin(nterm);
  for (size_t t = 0; t < nterm; ++t) {
    ll[t] = {rng() % nl, wires[rng() % ndistinct], {rng(), rng()}};
    lin[t] = {ll[t].c, ll[t].w, elt_t{ll[t].k[0], ll[t].k[1]}};
  }
  std::vector<elt_t> alphal(nl), alphaq(3 * p.nq);
  for (auto& e : alphal) e = elt_t{rng(), rng()};
  for (auto& e : alphaq) e = elt_t{rng(), rng()};
  const std::vector<size_t> lqc = {1, 2, 3};
  const size_t ld = p.dblock, nelt = p.nwqrow * ld;
  void* d_rows = nullptr;
  CK(lfgpu_malloc(c, nelt * 16, &d_rows));
  const zkp::Wire16 pol;
  const HostField F(c, field);
  std::vector<elt_t> got[2] = {std::vector<elt_t>(nelt), std::vector<elt_t>(nelt)};
  std::vector<double> ms[2];
  for (int pass = 0; pass < 8; ++pass)  // pass 0 warms both routes up (scratch growth, code load)
    for (int route = 0; route < 2; ++route) {
      CK(hipMemset(d_rows, 0, nelt * 16) != hipSuccess);
      CK(lfgpu_sync(c));
      const double t0 = zkp::now_ms();
      if (route == 0) {
        const LfLigeroTerms t{ll.data(), nterm, alphal.data(), nl, lqc.data(), alphaq.data()};
        CK(lf_ligero_a_rows_terms(c, field, &p, ld, &t, d_rows));
      } else {
        std::vector<uint64_t> idx;
        std::vector<elt_t> val;
        zkp::inner_product_sparse<zkp::Wire16>(F, p, lin, alphal, lqc, alphaq, idx, val);
        CK(lfgpu_ligero_inner_product_rows(c, field, p.w, p.r, ld, p.nwqrow, nullptr, 0, nullptr, idx.data(), val.data(), idx.size(), d_rows));
      }
      CK(lfgpu_sync(c));
      if (pass) ms[route].push_back(zkp::now_ms() - t0);
      CK(lfgpu_memcpy_d2h(c, got[route].data(), d_rows, nelt * 16));
    }
  const bool same = memcmp(got[0].data(), got[1].data(), nelt * 16) == 0;
  for (int route = 0; route < 2; ++route) {
    std::sort(ms[route].begin(), ms[route].end());
    printf("%-6s median %.3f ms (min %.3f, max %.3f) over %zu passes\n", route ? "host" : "device", ms[route][ms[route].size() / 2], ms[route].front(),
           ms[route].back(), ms[route].size());
  }
  printf("rows of the two routes: %s\n", same ? "identical" : "DIFFER");
  (void)pol;
  lfgpu_free(c, d_rows);
  lfgpu_shutdown(c);
  return same ? 0 : 1;
}
