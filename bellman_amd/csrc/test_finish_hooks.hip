// Test hook of the device proof assembly (include/bellman_hip_test.h): bh_groth16_assemble_many's contract computed by the
// host compilation of csrc/proof_finish.cuh - the text the kernels of proof_finish.hip compile
// (tests/test_proof_finish_cpu.py).  The verifying key comes through the C ABI, as for any caller.
#include <string.h>

#include "../../include/bellman_hip_test.h"
#include "proof_finish.cuh"

using namespace bh;

extern "C" {

int bh_test_proof_finish_host_vk(const void *vk5, const void *sums, const void *r, const void *s, size_t k, void *proofs_out,
                                 int32_t *rcs) {
  if (!vk5) return BH_ERR_INVALID_ARG;
  if (!k) return BH_OK;
  if (!sums || !r || !s || !proofs_out || !rcs) return BH_ERR_INVALID_ARG;
  FinishKey key;
  memcpy(&key, vk5, sizeof key);
  if (aff_is_identity(key.delta_g1) || aff_is_identity(key.delta_g2)) {   // prover.rs:320-324
    memset(proofs_out, 0, k * sizeof(FinishProof));
    for (size_t j = 0; j < k; j++) rcs[j] = BH_ERR_UNEXPECTED_IDENTITY;
    return BH_OK;
  }
  for (size_t j = 0; j < k; j++) {   // host buffers carry no alignment promise
    FinishSums m;
    fr_t rj, sj;
    FinishProof p;
    memcpy(&m, (const char *)sums + j * sizeof m, sizeof m);
    memcpy(&rj, (const char *)r + j * 32, 32);
    memcpy(&sj, (const char *)s + j * 32, 32);
    finish_proof_host(p, key, m, rj, sj);
    memcpy((char *)proofs_out + j * sizeof p, &p, sizeof p);
    rcs[j] = BH_OK;
  }
  return BH_OK;
}

int bh_test_proof_finish_host(bh_params *params, const void *sums, const void *r, const void *s, size_t k, void *proofs_out,
                              int32_t *rcs) {
  if (!params) return BH_ERR_INVALID_ARG;
  FinishKey key;
  const int rc = bh_groth16_params_vk(params, &key.alpha_g1, &key.beta_g1, &key.beta_g2, &key.delta_g1, &key.delta_g2);
  return rc != BH_OK ? rc : bh_test_proof_finish_host_vk(&key, sums, r, s, k, proofs_out, rcs);
}

}  // extern "C"
