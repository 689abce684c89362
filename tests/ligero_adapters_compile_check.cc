// ligero_adapters_compile_check.cc -- compile-only check that lfgpu::GpuLigeroProver / GpuLigeroVerifier
// (include/lfgpu_zk_adapters.h) take the reference's own argument types: LigeroParam, LigeroCommitment, LigeroProof,
// LigeroLinearConstraint<Field>[], LigeroHash, LigeroQuadraticConstraint[], Transcript and RandomEngine, for GF2_128 and Fp128.
// Compiled with `g++ -c` against the reference's headers by tests/test_ligero_adapters_compile.py; never run.
#include "algebra/fp_p128.h"
#include "gf2k/gf2_128.h"
#include "ligero/ligero_param.h"
#include "random/random.h"
#include "random/transcript.h"

#include "lfgpu_adapters.h"
#include "lfgpu_zk_adapters.h"

namespace {
template <class Field>
bool ligero_with_gpu_prover_and_verifier(const Field& F, const lfgpu::Context& ctx, const typename Field::Elt* W, const typename Field::Elt* b,
                                         const proofs::LigeroLinearConstraint<Field>* llterm, size_t nllterm,
                                         const proofs::LigeroQuadraticConstraint* lqc, proofs::RandomEngine& rng) {
  proofs::LigeroParam<Field> p(1000, 50, 4, 36, 4096);
  proofs::LigeroCommitment<Field> com;
  proofs::LigeroProof<Field> proof(&p);
  proofs::LigeroHash h{};
  proofs::Transcript tp((const uint8_t*)"test", 4), tv((const uint8_t*)"test", 4);
  lfgpu::GpuLigeroProver<Field> prover(ctx, p);
  prover.commit(com, tp, W, 0, lqc, rng, F);
  prover.prove(proof, tp, 15, nllterm, llterm, h, lqc, F);
  lfgpu::GpuLigeroVerifier<Field> verifier(ctx);
  lfgpu::GpuLigeroVerifier<Field>::receive_commitment(com, tv);
  const char* why = nullptr;
  return verifier.verify(&why, p, com, proof, tv, 15, nllterm, llterm, h, b, lqc, F);
}
}  // namespace

bool lfgpu_ligero_adapters_compile_check(const lfgpu::Context& ctx, proofs::RandomEngine& rng) {
  static const proofs::GF2_128<> gf;
  static const proofs::GF2_128<5> gf5;
  static const proofs::Fp128<> fp;
  return ligero_with_gpu_prover_and_verifier<proofs::GF2_128<>>(gf, ctx, nullptr, nullptr, nullptr, 0, nullptr, rng) &&
         ligero_with_gpu_prover_and_verifier<proofs::GF2_128<5>>(gf5, ctx, nullptr, nullptr, nullptr, 0, nullptr, rng) &&
         ligero_with_gpu_prover_and_verifier<proofs::Fp128<>>(fp, ctx, nullptr, nullptr, nullptr, 0, nullptr, rng);
}
