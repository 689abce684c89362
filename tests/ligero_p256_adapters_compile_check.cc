// ligero_p256_adapters_compile_check.cc -- compile-only check that lfgpu::GpuLigeroProver / GpuLigeroVerifier
// (include/lfgpu_zk_adapters.h) take the reference's own argument types over Fp256Base: LigeroParam, LigeroCommitment,
// LigeroProof, LigeroLinearConstraint<Fp256Base>[] (a 48-byte record: lfgpu_ligero_llterm256), LigeroHash,
// LigeroQuadraticConstraint[], Transcript and RandomEngine.  Compiled with `g++ -c` against the reference's headers by
// tests/test_ligero_p256_adapters_compile.py; never run.
#include "ec/p256.h"
#include "ligero/ligero_param.h"
#include "random/random.h"
#include "random/transcript.h"

#include "lfgpu_adapters.h"
#include "lfgpu_zk_adapters.h"

namespace {
using Field = proofs::Fp256Base;
static_assert(sizeof(proofs::LigeroLinearConstraint<Field>) == sizeof(lfgpu_ligero_llterm256), "the reference's term record is the C ABI's");
static_assert(lfgpu::field_id<Field>() == LFGPU_FIELD_P256, "Fp256Base is field id 1");

bool ligero_with_gpu_prover_and_verifier(const Field& F, const lfgpu::Context& ctx, const Field::Elt* W, const Field::Elt* b,
                                         const proofs::LigeroLinearConstraint<Field>* llterm, size_t nllterm, const proofs::LigeroQuadraticConstraint* lqc,
                                         proofs::RandomEngine& rng) {
  proofs::LigeroParam<Field> p(300, 30, 4, 18);  // the statement of tests/golden/ligero_p256_vector.bin
  proofs::LigeroCommitment<Field> com;
  proofs::LigeroProof<Field> proof(&p);
  proofs::LigeroHash h{};
  proofs::Transcript tp((const uint8_t*)"test", 4), tv((const uint8_t*)"test", 4);
  lfgpu::GpuLigeroProver<Field> prover(ctx, p);
  prover.commit(com, tp, W, 0, lqc, rng, F);
  prover.prove(proof, tp, 7, nllterm, llterm, h, lqc, F);
  lfgpu::GpuLigeroVerifier<Field> verifier(ctx);
  lfgpu::GpuLigeroVerifier<Field>::receive_commitment(com, tv);
  const char* why = nullptr;
  return verifier.verify(&why, p, com, proof, tv, 7, nllterm, llterm, h, b, lqc, F);
}
}  // namespace

bool lfgpu_ligero_p256_adapters_compile_check(const lfgpu::Context& ctx, proofs::RandomEngine& rng) {
  return ligero_with_gpu_prover_and_verifier(proofs::p256_base, ctx, nullptr, nullptr, nullptr, 0, nullptr, rng);
}
