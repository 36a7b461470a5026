// kit4b_amd/csrc/k4_contam_rule.h -- the rule of kalign's contaminant flank trimming (`-H`), stated once for the kernel of
// k4_contam.hip and for the host (k4_contam_match_host):
//   CContaminants::MatchContaminants  libkit4b/Contaminants.cpp:1243-1325, over the trie of IndexContamSeq :820 / RecursiveMatch :977
//
// The trie is a search structure only.  A node at depth d exists because some contaminant of its class is longer than d, and its
// MaxContamSfxLen is the largest remainder of any contaminant through it, so a walk of L steps survives the length test of every
// node exactly when one contaminant of at least L bases spells that path.  What MatchContaminants returns is therefore the largest
// L, from min(read length, longest contaminant of the class) down to the minimum overlap, for which SOME contaminant of the class
// with length >= L overlaps the read end over L bases with at most one substitution (kalign passes AllowSubsRate 1 and the code
// clamps with min(1, ..), so the allowance is one at every L):
//   5' classes: the contaminant's last L bases against the read's first L;  3' classes: its first L against the read's last L.
//   A read N always costs a substitution; a contaminant N matches anything but a read N; a read byte that is neither a base nor N
//   (eBaseInDel) equals no contaminant base, so it costs one unless the contaminant has N there.
//
// Both sides are packed one bit per base and plane into 256 positions (4 x 64-bit words per plane): planes 0 / 1 the two bits of
// a base, plane 2 "is N", plane 3 (reads only) "neither base nor N".  Of the two sequences of an overlap one is RIGHT aligned
// (position 256 - n + k holds element k of its n) and one LEFT aligned (position k holds element k):
//   5' classes: contaminant right (its suffix ends at 255), read head left;  3' classes: read tail right, contaminant left.
// An overlap of L is then: the right-aligned side shifted down by 256 - L, XOR, mask to L bits, popcount.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define K4_CONTAM_MIN_LEN 4        // cMinContaminantLen, libkit4b/Contaminants.h:11
#define K4_CONTAM_MAX_LEN 200      // cMaxContaminantLen :12
#define K4_CONTAM_MAX_ENTRIES 1600 // cMaxNumContaminants :13
#define K4_CONTAM_MIN_READ 20      // cMinContamQuerySeqLen :8: a shorter read is not examined
#define K4_CONTAM_MAX_READ 2000    // cMaxContamQuerySeqLen :9: nor is a longer one
#define K4_CONTAM_WORDS 4
#define K4_CONTAM_PLANES 4

// a read byte (etSeqBase in bits 0..2, flags and the 4-bit quality above): which planes carry a 1 for it
__host__ __device__ inline uint32_t k4c_read_planes(uint8_t b) {
  const uint32_t v = b & 7u;
  return v < 4u ? v : v == 4u ? 4u : 8u;
}

// the read base that sits at position p of the packed read end (-1: none): the first / last min(len, 200) bases
__host__ __device__ inline int64_t k4c_read_index(bool five, uint32_t len, uint32_t p) {
  const uint32_t m = len < (uint32_t)K4_CONTAM_MAX_LEN ? len : (uint32_t)K4_CONTAM_MAX_LEN;
  if (five) return p < m ? (int64_t)p : -1;
  return p >= 256u - m && p < 256u ? (int64_t)len - 256 + (int64_t)p : -1;
}

// word k of plane `plane` of v, v shifted down by s positions (0 <= s < 256)
template <class V>
__host__ __device__ inline uint64_t k4c_shr(const V& v, uint32_t plane, uint32_t s, uint32_t k) {
  const uint32_t q = (s >> 6) + k, r = s & 63u;
  const uint64_t lo = q < (uint32_t)K4_CONTAM_WORDS ? v.word(plane, q) : 0ull;
  if (r == 0u) return lo;
  const uint64_t hi = q + 1u < (uint32_t)K4_CONTAM_WORDS ? v.word(plane, q + 1u) : 0ull;
  return (lo >> r) | (hi << (64u - r));
}

__host__ __device__ inline uint32_t k4c_popc(uint64_t x) {
#ifdef __HIP_DEVICE_COMPILE__
  return (uint32_t)__popcll(x);
#else
  return (uint32_t)__builtin_popcountll(x);
#endif
}

// substitutions an overlap of L (1..200) costs, counted as far as 2: the rule accepts 0 and 1.  R, C: word(plane, k) of the packed
// read end and of the contaminant
template <class R, class C>
__host__ __device__ inline uint32_t k4_contam_subs(const R& read, const C& contam, uint32_t L, bool five) {
  const uint32_t s = 256u - L;
  uint32_t subs = 0;
  for (uint32_t k = 0; k * 64u < L; k++) {
    uint64_t r0, r1, rn, rx, c0, c1, cn;
    if (five) {
      c0 = k4c_shr(contam, 0, s, k); c1 = k4c_shr(contam, 1, s, k); cn = k4c_shr(contam, 2, s, k);
      r0 = read.word(0, k); r1 = read.word(1, k); rn = read.word(2, k); rx = read.word(3, k);
    } else {
      r0 = k4c_shr(read, 0, s, k); r1 = k4c_shr(read, 1, s, k); rn = k4c_shr(read, 2, s, k); rx = k4c_shr(read, 3, s, k);
      c0 = contam.word(0, k); c1 = contam.word(1, k); cn = contam.word(2, k);
    }
    uint64_t mm = rn | (~cn & (rx | (r0 ^ c0) | (r1 ^ c1)));
    const uint32_t left = L - k * 64u;
    if (left < 64u) mm &= (1ull << left) - 1ull;
    subs += k4c_popc(mm);
    if (subs > 1u) return 2u;
  }
  return subs;
}
