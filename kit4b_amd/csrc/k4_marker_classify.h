// kit4b_amd/csrc/k4_marker_classify.h -- the per-locus rule of kalign's marker sequences (CKAligner::OutputSNPs, KAligner.cpp:7513-7536),
// written once for the kernel (k4k_snp_markers) and for the host (k4_marker_classify_host): the base a locus contributes to a marker
// sequence, or why the marker is rejected there, and whether the locus counts as polymorphic.
//
// The proportions are IEEE doubles compared with the reference's own literals (0.1, 0.9) and with 1.0 - threshold computed as the
// reference computes it; division and comparison stay in its order (see k4_pba_classify.h for why no integer restatement).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define K4_MARKER_NO_COVERAGE (-1)  // fewer than MinSNPreads bases at the locus: the walk stops, the marker is rejected (:7515)
#define K4_MARKER_NO_ALLELE (-2)    // too polymorphic for the reference base and no allele reaches 1 - threshold (:7534)

// n_ref / n_non: NumRefBases / NumNonRefBases; by_base: NonRefBaseCnts[A, C, G, T, N]; ref_base: the target's symbol (pSNP->RefBase).
// Returns the base (0..3, 4 = N) or one of the two rejections; *polymorphic = 1 when the locus adds to NumPolymorphicSites.
__host__ __device__ inline int k4_marker_base(uint32_t n_ref, uint32_t n_non, const uint32_t (&by_base)[5], uint32_t ref_base, int min_snp_reads,
                                              double poly_thres, int* polymorphic) {
  *polymorphic = 0;
  const int tot = (int)(n_non + n_ref);
  if (tot < min_snp_reads || tot <= 0) return K4_MARKER_NO_COVERAGE;
  double prop = (double)n_non / tot;
  if (prop <= poly_thres) {  // no more than the polymorphic threshold: the reference base stands
    if (prop > 0.1) *polymorphic = 1;
    return (int)(ref_base > 4 ? 4 : ref_base);
  }
  for (int b = 0; b < 5; b++)  // the first allele that accounts for nearly all bases there
    if (by_base[b] > 0 && (prop = (double)by_base[b] / tot) >= (1.0 - poly_thres)) {
      if (prop < 0.9) *polymorphic = 1;
      return b;
    }
  return K4_MARKER_NO_ALLELE;
}
