// kit4b_amd/csrc/k4_pba_classify.h -- genpba's per-locus rule (CKAligner::OutputSNPs, KAligner.cpp:7262-7302), written once for the
// kernel (k4k_pba_classify) and for the host (k4_pba_classify_host): the byte of four 2-bit allele scores, A in bits 7..6, C in 5..4,
// G in 3..2, T in 1..0, and the coverage it is taken over.
//
// The proportions are IEEE doubles compared with the reference's own literals (KAligner.h:124-129).  0.35, 0.20, 0.70 and 0.30 have
// no exact binary form, so an integer restatement (20 c >= 7 n, ...) would decide the loci whose proportion lands on a threshold
// by the exact rational instead of by the rounded quotient against the rounded literal: 7 / 20.0 >= 0.35 holds only because both
// round to the same double.  Division and comparison stay as the reference has them.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

// n_ref / n_non: NumRefBases / NumNonRefBases; by_base: NonRefBaseCnts[A, C, G, T, N]; ref_base: the target's symbol (0..3; anything
// else matches no allele).  *coverage = the bases counted there without the indeterminate ones.
__host__ __device__ inline uint8_t k4_pba_byte(uint32_t n_ref, uint32_t n_non, const uint32_t (&by_base)[5], uint32_t ref_base, uint32_t* coverage) {
  const uint32_t cov = n_non + n_ref - by_base[4];
  *coverage = cov;
  if (cov == 0) return 0;
  uint32_t pba = 0;
  for (uint32_t b = 0; b < 4; b++) {
    pba <<= 2;
    const uint32_t n = b == ref_base ? n_ref : by_base[b];
    if (n == 0) continue;  // (0.0 reaches no threshold: most alleles of most loci, and no division for them)
    const double prop = n / (double)cov;
    if (cov >= 5) {
      if (prop >= 0.75) pba |= 3;        // cScorePBA3MinProp
      else if (prop >= 0.35) pba |= 2;   // cScorePBA2MinProp
      else if (prop >= 0.20) pba |= 1;   // cScorePBA1MinProp
    } else {
      if (prop >= 0.70) pba |= 2;        // cScorePBA2MinLCProp
      else if (prop >= 0.30) pba |= 1;   // cScorePBA1MinLCProp
    }
  }
  return (uint8_t)pba;
}
