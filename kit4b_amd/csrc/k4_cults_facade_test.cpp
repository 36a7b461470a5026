// kit4b_amd/csrc/k4_cults_facade_test.cpp -- CSfxArray::GenKMerCultThreadRange / GenKMerCultsCnts of include/k4_sfxarray.hpp as
// CMarkerKMers::LocKMers uses them (ngskit4b/MarkerKMers.cpp:449-476, :872-876): the range is partitioned for the given number of threads, each
// active thread sweeps its range with a recording callback, all at once,, and the callbacks in range order are compared with the recorded ones
// of the reference (tests/golden/make_golden_cults.py gives the byte form).  Then, unless the fourth argument is "-", a callback that
// answers -7 on its third call, the parameter errors and the homozygotic call.
//   k4_cults_facade_test <index.sfx> <callbacks.bin> <located> <abort_callbacks.bin | -> <MinCultivars> <threads, 1..4>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <thread>
#include "k4_facade_test_util.h"

static const int P = 12, S = 6;

struct Rec {
  std::vector<uint8_t> bytes;
  int n_cb = 0, abort_at = 0;
};
template <typename T>
static void put(std::vector<uint8_t>& v, T x) {
  const uint8_t* p = (const uint8_t*)&x;
  v.insert(v.end(), p, p + sizeof(T));
}
static int record(void* pThis, tsKMerCultsCnts* p) {
  Rec* r = (Rec*)pThis;
  uint32_t nnz = 0, dense_ok = 1;
  for (uint32_t i = 0; i < (uint32_t)cMaxCultivars; i++) {
    const tsKMerCultDist& d = p->CultCnts[i];
    if (i < p->TotCultivars) { if (d.EntryID != i + 1) dense_ok = 0; if (d.SenseCnts || d.AntisenseCnts) nnz++; }
    else if (d.EntryID || d.SenseCnts || d.AntisenseCnts) dense_ok = 0;
  }
  put<uint64_t>(r->bytes, p->SenseCnts); put<uint64_t>(r->bytes, p->AntisenseCnts); put<uint32_t>(r->bytes, p->NumCultivars);
  put<uint32_t>(r->bytes, p->TotCultivars); put<uint32_t>(r->bytes, dense_ok); put<uint32_t>(r->bytes, nnz);
  r->bytes.insert(r->bytes.end(), p->KMerSeq, p->KMerSeq + P + S + 1);
  for (uint32_t i = 0; i < p->TotCultivars; i++) {
    const tsKMerCultDist& d = p->CultCnts[i];
    if (d.SenseCnts || d.AntisenseCnts) { put<uint32_t>(r->bytes, d.EntryID); put<uint32_t>(r->bytes, d.SenseCnts); put<uint32_t>(r->bytes, d.AntisenseCnts); }
  }
  return ++r->n_cb == r->abort_at ? -7 : 0;
}
static std::vector<uint8_t> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int min_cult = atoi(argv[5]);
  CSfxArray sfx;
  if (K4FtOpen(&sfx, argv[1]) != 0) { fprintf(stderr, "open failed\n"); return 1; }
  const bool rest = std::string(argv[4]) != "-";
  const std::vector<uint8_t> want = slurp(argv[2]), want_abort = rest ? slurp(argv[4]) : std::vector<uint8_t>();
  const long long want_located = atoll(argv[3]);
  const int n_threads = atoi(argv[6]);
  if (n_threads < 1 || n_threads > 4) return 2;
  int64_t starts[4], ends[4], located[4] = {0, 0, 0, 0};
  int active = 0;
  int64_t start = 0, end = 0;
  for (; active < n_threads; active++) {
    if (sfx.GenKMerCultThreadRange(P, active + 1, n_threads, start, &end) < 1) break;
    starts[active] = start; ends[active] = end;
    start = end + 1;
  }
  Rec recs[4];
  std::vector<std::thread> th;
  for (int t = 0; t < active; t++)
    th.emplace_back([&, t] { located[t] = sfx.GenKMerCultsCnts(false, starts[t], ends[t], P, S, min_cult, 0, &recs[t], record); });
  for (std::thread& t : th) t.join();
  std::vector<uint8_t> got;
  long long total = 0;
  for (int t = 0; t < active; t++) { got.insert(got.end(), recs[t].bytes.begin(), recs[t].bytes.end()); total += located[t]; }
  printf("threads %d active %d located %lld callbacks %s\n", n_threads, active, total, got == want && total == want_located ? "match" : "DIFFER");
  if (!rest) return got == want && total == want_located ? 0 : 1;
  Rec ab;
  ab.abort_at = 3;
  const int64_t rc = sfx.GenKMerCultsCnts(false, 0, 0, P, S, 1, 0, &ab, record);
  printf("abort %lld after %d %s\n", (long long)rc, ab.n_cb, ab.bytes == want_abort ? "match" : "DIFFER");
  Rec none;
  const int64_t e1 = sfx.GenKMerCultsCnts(false, 0, 0, 4, S, 1, 0, &none, record), e2 = sfx.GenKMerCultsCnts(false, 0, 0, P, S, 6, 0, &none, record),
                e3 = sfx.GenKMerCultsCnts(false, -1, 0, P, S, 1, 0, &none, record), e4 = sfx.GenKMerCultsCnts(false, 0, 0, P, S, 1, 1, &none, record);
  printf("errors %lld %lld %lld unsupported %lld\n", (long long)e1, (long long)e2, (long long)e3, (long long)e4);
  return none.n_cb == 0 ? 0 : 1;
}
