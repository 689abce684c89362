// Host-only harness of tests/test_ligero_layout_host.py: lig::layout (csrc/ligero_layout.h) for GF(2^128) (k = 4), Fp128 and
// Fp256Base behind one C function.  Compiled with hipcc --cuda-host-only and linked against liblfgpu.so for the host helpers the
// header calls (the GF(2^128) constants, the Fp128 Montgomery conversion); no device is opened.
// Elements cross this ABI as their to_bytes_field images (canonical little-endian values), never in Montgomery form.
//
// With -DHLL_MAIN the file is a stand-alone program that runs one layout per field with `exact` on and off, whole and as the empty
// slab, for a run under the host sanitizers:
//   hipcc --cuda-host-only -O1 -g -std=c++17 -DHLL_MAIN -Xarch_host -fsanitize=address,undefined -o hll_main tests/host_ligero_layout.hip \
//         -Llongfellow-zk_amd -l:liblfgpu.so -Wl,-rpath,$PWD/longfellow-zk_amd && ./hll_main
#include "../longfellow-zk_amd/csrc/ligero_layout.h"

namespace {
// canonical bytes <-> the element images the layout works on
bool get(const lig::Host16& hp, const uint8_t* b, elt_t& e) {
  memcpy(&e, b, 16);
  if (hp.field == LFGPU_FIELD_GF2_128) return true;
  if (!h_fp_fits(e)) return false;
  e = h_fp_to_mont(e);
  return true;
}
void put(const lig::Host16& hp, elt_t e, uint8_t* b) {
  if (hp.field != LFGPU_FIELD_GF2_128) e = fp_from_mont(e);
  memcpy(b, &e, 16);
}
bool get(const lig::Host32&, const uint8_t* b, elt32_t& e) { return h256_of_bytes(b, e); }
void put(const lig::Host32&, const elt32_t& e, uint8_t* b) { h256_to_bytes(e, b); }

template <class H>
int run(const H& hp, const lfgpu_ligero_param* p, const uint8_t* W, size_t subfield_boundary, const size_t* lqc, lfgpu_rng_fn rng, void* user, int exact,
        size_t row_lo, size_t row_hi, uint8_t* rows_out, uint8_t* nonces_out, char* err) {
  using E = typename H::E;
  std::vector<E> w(p->nw), img((row_hi - row_lo) * p->dblock);
  for (size_t i = 0; i < p->nw; ++i)
    if (!get(hp, W + sizeof(E) * i, w[i])) return -1;
  const int rc = lig::layout(hp, *p, w.data(), subfield_boundary, lqc, rng, user, exact != 0, row_lo, row_hi, img.data(), nonces_out, err);
  for (size_t i = 0; i < img.size(); ++i) put(hp, img[i], rows_out + sizeof(E) * i);
  return rc;
}
}  // namespace

// lig::layout of rows [row_lo, row_hi): W holds p->nw canonical elements, rows_out takes (row_hi - row_lo) * dblock of them,
// nonces_out (32 * block_ext bytes) may be null, err has 256 bytes.  Returns the layout's code, or -1 for a W element >= p.
extern "C" int hll_layout(int field, const lfgpu_ligero_param* p, const uint8_t* W, size_t subfield_boundary, const size_t* lqc, lfgpu_rng_fn rng, void* user,
                          int exact, size_t row_lo, size_t row_hi, uint8_t* rows_out, uint8_t* nonces_out, char* err) {
  if (field == LFGPU_FIELD_P256) return run(lig::Host32(), p, W, subfield_boundary, lqc, rng, user, exact, row_lo, row_hi, rows_out, nonces_out, err);
  static GfHostCtx g;  // (lf_gf_ctx_build fills it once)
  if (field == LFGPU_FIELD_GF2_128 && !lf_gf_ctx_build(&g, 4)) return -1;
  return run(lig::Host16{field, 4, &g}, p, W, subfield_boundary, lqc, rng, user, exact, row_lo, row_hi, rows_out, nonces_out, err);
}

#ifdef HLL_MAIN
// an engine whose every 5th 16-byte chunk is 0xff..ff: both prime fields reject attempts (>= p) inside every row
static void lcg(void* user, uint8_t* buf, size_t n) {
  uint64_t* s = (uint64_t*)user;
  for (size_t i = 0; i < n; ++i) {
    s[0] = s[0] * 6364136223846793005ull + 1442695040888963407ull;
    buf[i] = (s[1]++ / 16) % 5 == 4 ? 0xff : (uint8_t)(s[0] >> 56);
  }
}
int main() {
  const int fields[3] = {LFGPU_FIELD_GF2_128, LFGPU_FIELD_FP128, LFGPU_FIELD_P256};
  for (int field : fields) {
    const size_t esz = field == LFGPU_FIELD_P256 ? 32 : 16, nw = 40, nq = 10, sfb = field == LFGPU_FIELD_GF2_128 ? 17 : 0;
    lfgpu_ligero_param p;
    if (lfgpu_ligero_param_init(&p, field, 4, nw, nq, 4, 3, 63)) return 1;
    std::vector<uint8_t> W(nw * esz, 0), rows(p.nrow * p.dblock * esz), nonces(32 * p.block_ext);
    for (size_t i = 20; i < 30; ++i) W[i * esz] = 1;  // W[l2] = W[l0] * W[l1] over values 0 and 1
    std::vector<size_t> lqc;
    for (size_t i = 0; i < nq; ++i) lqc.insert(lqc.end(), {i, 20 + i, i});
    for (int exact = 0; exact < 2; ++exact)
      for (size_t hi : {p.nrow, (size_t)0, p.iw + 1}) {
        uint64_t seed[2] = {7, 0};
        char err[256] = {0};
        const size_t lo = hi == p.nrow ? 0 : hi ? hi - 1 : 0;
        const int rc = hll_layout(field, &p, W.data(), sfb, lqc.data(), lcg, seed, exact, lo, hi, rows.data(), hi ? nonces.data() : nullptr, err);
        printf("field %d exact %d rows [%zu, %zu): rc %d, %llu bytes drawn %s\n", field, exact, lo, hi, rc, (unsigned long long)seed[1], err);
        if (rc) return 1;
      }
  }
  return 0;
}
#endif
