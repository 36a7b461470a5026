"""k4d_revcomp_words (kit4b_amd/csrc/k4_revcomp.h) on the host: the reverse-complement words a later phase of the step kernels
rebuilds from a lean survivor row, held against a packer that works base by base -- every length 1..512 in every length class
that takes it (4, 5, 8 and 16 words a strand), random bases, both the contiguous layout and a strided one as the kernels' LDS
columns have it.  The header is compiled with its function qualifier made empty; no GPU and no library is needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#define K4_RC_FN static inline
#include "k4_revcomp.h"

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 32); }

// the exact packer: base b of the sequence goes to bits 63 - 2 * (b % 32) .. of word b / 32, nothing else is set
static void pack(const uint8_t* s, int len, uint64_t* w, int nch) {
  for (int c = 0; c <= nch; c++) w[c] = 0;
  for (int b = 0; b < len; b++) w[b >> 5] |= (uint64_t)s[b] << (62 - 2 * (b & 31));
}

template <int NCH>
static long check_class(int* n_checked) {
  constexpr int STRIDE = 7;
  long bad = 0;
  for (int len = 1; len <= 32 * NCH; len++)
    for (int rep = 0; rep < 8; rep++) {
      uint8_t s[512], r[512];
      for (int b = 0; b < len; b++) s[b] = rep == 0 ? 0 : rep == 1 ? 3 : (uint8_t)(rnd() & 3);  // all A and all T among them
      for (int b = 0; b < len; b++) r[b] = (uint8_t)(3 - s[len - 1 - b]);
      uint64_t fwd[NCH + 1], want[NCH + 1], got[NCH], fs[(NCH + 1) * STRIDE], gs[NCH * STRIDE];
      pack(s, len, fwd, NCH);
      pack(r, len, want, NCH);
      memset(got, 0xA5, sizeof got);
      k4d_revcomp_words<NCH, 1>(fwd, len, got);
      memset(fs, 0x5A, sizeof fs);
      memset(gs, 0xA5, sizeof gs);
      for (int c = 0; c <= NCH; c++) fs[c * STRIDE] = fwd[c];
      k4d_revcomp_words<NCH, STRIDE>(fs, len, gs);
      for (int c = 0; c < NCH; c++)
        if (got[c] != want[c] || gs[c * STRIDE] != want[c]) {
          if (bad++ < 8) printf("NCH %d len %d rep %d word %d: got %016llx / %016llx want %016llx\n", NCH, len, rep, c,
                                (unsigned long long)got[c], (unsigned long long)gs[c * STRIDE], (unsigned long long)want[c]);
        }
      for (int q = 0; q < NCH * STRIDE; q++)  // nothing beside the NCH words is written
        if (q % STRIDE && gs[q] != 0xA5A5A5A5A5A5A5A5ull) bad++;
      (*n_checked)++;
    }
  return bad;
}

int main() {
  // k4d_rev2 itself: the 32 two-bit groups in reverse order
  for (int q = 0; q < 1000; q++) {
    const uint64_t x = ((uint64_t)rnd() << 32) | rnd();
    uint64_t y = 0;
    for (int g = 0; g < 32; g++) y |= ((x >> (2 * g)) & 3) << (62 - 2 * g);
    if (k4d_rev2(x) != y) { printf("k4d_rev2(%016llx)\n", (unsigned long long)x); return 1; }
  }
  int n = 0;
  const long bad = check_class<4>(&n) + check_class<5>(&n) + check_class<8>(&n) + check_class<16>(&n);
  printf("checked %d bad %ld\n", n, bad);
  return bad ? 1 : 0;
}
"""


def test_revcomp_words_equal_the_exact_packer(tmp_path):
    src = tmp_path / "revcomp_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "revcomp_host"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "kit4b_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True, timeout=120)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "checked %d bad 0" % (8 * 32 * (4 + 5 + 8 + 16)), p.stdout
