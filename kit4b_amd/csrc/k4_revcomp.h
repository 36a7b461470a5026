// kit4b_amd/csrc/k4_revcomp.h -- the reverse-complement words of a packed read from its forward words and its length: what a lean
// survivor row (K4_LEAN_ROW, k4_align_common.h) leaves out and the later phases of k4k_align_step rebuild in the lane's LDS column.
// Included by k4_align_common.h; it needs nothing of the device, so that a host program can hold it against a packer that works
// base by base (tests/test_revcomp_cpu.py: K4_RC_FN empty, every length 1..512).
#pragma once
#include <stdint.h>

#ifndef K4_RC_FN
#define K4_RC_FN __device__ __forceinline__
#endif

// reverse the order of the 32 two-bit groups of a word
K4_RC_FN uint64_t k4d_rev2(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint64_t y = __brevll(x);
#else
  uint64_t y = x;
  y = ((y >> 1) & 0x5555555555555555ull) | ((y & 0x5555555555555555ull) << 1);
  y = ((y >> 2) & 0x3333333333333333ull) | ((y & 0x3333333333333333ull) << 2);
  y = ((y >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((y & 0x0F0F0F0F0F0F0F0Full) << 4);
  y = __builtin_bswap64(y);
#endif
  return ((y & 0x5555555555555555ull) << 1) | ((y >> 1) & 0x5555555555555555ull);
}

// fwd[c * STRIDE], c = 0..NCH: the forward words of a read of len bases (1 <= len <= 32 * NCH), 32 bases a word, first base in the
// top two bits, zero behind the last base; word NCH is the zero pad word.  Writes rc[c * STRIDE], c = 0..NCH-1, in the same form:
// rc bases [32c, 32c + 32) are the complement of the forward bases [len - 32(c + 1), len - 32c) in reverse order -- one funnel
// shift over two forward words, a bit reversal with the bits of each pair swapped back, a complement and the end mask per word.
// (In a step kernel both are the lane's LDS column, STRIDE = the block size: the word index depends on the length, which LDS
// addresses take and registers would not.)
template <int NCH, int STRIDE>
K4_RC_FN void k4d_revcomp_words(const uint64_t* fwd, int len, uint64_t* rc) {
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    uint64_t r = 0;
    if (32 * c < len) {
      const int o = len - 32 * (c + 1);
      uint64_t f;
      if (o >= 0) {
        const int w = o >> 5, sh = 2 * (o & 31);
        const uint64_t hi = fwd[w * STRIDE];
        f = sh ? (hi << sh) | (fwd[(w + 1) * STRIDE] >> (64 - sh)) : hi;
      } else
        f = fwd[0] >> (2 * (-o));  // fewer than 32 bases left: they sit at the low end, zeros above
      const int nb = len - 32 * c;  // bases of this word
      r = k4d_rev2(~f) & (nb >= 32 ? ~0ull : ~(~0ull >> (2 * nb)));
    }
    rc[c * STRIDE] = r;
  }
}
