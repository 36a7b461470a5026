"""kit4b_amd/csrc/k4_search_arith.h on the host: the index arithmetic the six search-call families share, compiled with its function
qualifier made empty and held against linear scans.  No GPU and no library is needed.

k4d_last_le      tables of 1, 2, 3, 63, 64 and 65 ascending offsets that start at 0, hold repeated values (empty runs) and end with
                 the total; every key from 0 to one past the last value; the answer of a scan from the front
k4d_runs_locate  a layout of 64 runs whose takes come from {0, 1, 63, 64, 65}: every candidate, with the search's upper end at lane
                 63 and at the last run that has a candidate, against the scan and against the loop the helper replaced
k4s_launch_windows  totals {0, 1, L-1, L, L+1, 2L, 2L+1} for L in {1, 64, 16384}: windows ascending, disjoint, none empty, none
                 above L, together [0, total); no call for total 0"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include <vector>
#define K4_SA_FN static inline
#include "k4_search_arith.h"

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 32); }

// the loop k4d_runs_locate was before it was written on k4d_last_le
static void old_runs_locate(uint32_t g, uint32_t hi, const uint32_t* g_pre, uint32_t& item, uint32_t& occ) {
  uint32_t lo = 0;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (g_pre[mid] <= g) lo = mid; else hi = mid - 1;
  }
  item = lo;
  occ = g - g_pre[lo];
}

int main() {
  long bad = 0, keys = 0, cands = 0, windows = 0;
  // k4d_last_le
  const int sizes[6] = {1, 2, 3, 63, 64, 65};
  for (int si = 0; si < 6; si++)
    for (int rep = 0; rep < 6; rep++) {
      const int n = sizes[si];
      std::vector<uint64_t> t((size_t)n);
      t[0] = 0;
      // rep 0: every run empty; rep 1: runs of one; else a mix of empty runs, runs of one and longer ones
      for (int i = 1; i < n; i++) t[(size_t)i] = t[(size_t)i - 1] + (rep == 0 ? 0u : rep == 1 ? 1u : (rnd() % 3 == 0 ? 0u : 1u + rnd() % 70));
      for (uint64_t key = 0; key <= t[(size_t)n - 1] + 1; key++) {
        uint32_t want = 0;
        for (uint32_t i = 0; i < (uint32_t)n; i++)
          if (t[i] <= key) want = i;
        const uint32_t got = k4d_last_le((uint32_t)n, key, [&](uint32_t i) { return t[i]; });
        const int64_t got64 = k4d_last_le((int64_t)n, key, [&](int64_t i) { return t[(size_t)i]; });  // (the span table's index type)
        if (got != want || got64 != (int64_t)want) {
          if (bad++ < 8) printf("last_le n %d rep %d key %llu: got %u / %lld want %u\n", n, rep, (unsigned long long)key, got, (long long)got64, want);
        }
        keys++;
      }
    }
  // k4d_runs_locate
  const uint32_t takes[5] = {0, 1, 63, 64, 65};
  for (int rep = 0; rep < 12; rep++) {
    uint32_t g_pre[65], take[64], last_run = 0;
    for (int i = 0; i < 64; i++) {
      take[i] = rep < 5 ? takes[rep] : takes[rnd() % 5];
      if (rep == 5 && i != 17) take[i] = 0;   // one run alone
      if (rep == 6 && i >= 40) take[i] = 0;   // nothing behind run 39
    }
    g_pre[0] = 0;
    for (int i = 0; i < 64; i++) {
      g_pre[i + 1] = g_pre[i] + take[i];
      if (take[i]) last_run = (uint32_t)i;
    }
    for (uint32_t g = 0; g < g_pre[64]; g++) {
      uint32_t want_item = 0;
      for (uint32_t i = 0; i < 64; i++)
        if (g_pre[i] <= g) want_item = i;
      const uint32_t his[2] = {63u, last_run};
      for (int h = 0; h < 2; h++) {
        uint32_t item, occ, o_item, o_occ;
        k4d_runs_locate(g, his[h], g_pre, item, occ);
        old_runs_locate(g, his[h], g_pre, o_item, o_occ);
        if (item != want_item || occ != g - g_pre[want_item] || occ >= take[item] || item != o_item || occ != o_occ) {
          if (bad++ < 8) printf("runs_locate rep %d g %u hi %u: got (%u, %u) was (%u, %u) want run %u\n", rep, g, his[h], item, occ, o_item, o_occ, want_item);
        }
      }
      cands++;
    }
  }
  // k4s_launch_windows
  const uint64_t Ls[3] = {1, 64, 16384};
  for (int li = 0; li < 3; li++) {
    const uint64_t L = Ls[li];
    const uint64_t totals[7] = {0, 1, L - 1, L, L + 1, 2 * L, 2 * L + 1};
    for (int ti = 0; ti < 7; ti++) {
      uint64_t next = 0, calls = 0;
      bool ok = true;
      k4s_launch_windows(totals[ti], L, [&](uint64_t k0, uint64_t k1) {
        ok = ok && k0 == next && k1 > k0 && k1 - k0 <= L && k1 <= totals[ti];
        next = k1;
        calls++;
      });
      if (!ok || next != totals[ti] || calls != (totals[ti] + L - 1) / L) {
        if (bad++ < 8) printf("launch_windows total %llu L %llu: %llu calls, covered %llu\n", (unsigned long long)totals[ti], (unsigned long long)L,
                              (unsigned long long)calls, (unsigned long long)next);
      }
      windows += (long)calls;
    }
  }
  printf("keys %ld candidates %ld windows %ld bad %ld\n", keys, cands, windows, bad);
  return bad || !keys || !cands || !windows ? 1 : 0;
}
"""


def test_search_arith_equals_linear_scans(tmp_path):
    src = tmp_path / "search_arith_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "search_arith_host"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "kit4b_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True, timeout=120)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("bad 0"), p.stdout
