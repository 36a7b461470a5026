// kit4b_amd/csrc/k4_hamming_facade_test.cpp -- include/k4_sfxarray.hpp's LocateSfxHammings / LocateHammings the way
// RestrictedHammingThread calls CSfxArray's (ngskit4b/hammings.cpp:1692-1694: each worker thread asks for its own span).
// usage: k4_hamming_facade_test index.sfx cases.txt
// cases.txt, per case: "form rhamm both klen nth mn mx iib entry loci len", form 0 = LocateSfxHammings, 1 = LocateHammings whose
// sequence follows as one word of digits; then len expected bytes (decimal; 255 = left as it was).
// Eight threads run every case at once, each starting at a different one, into arrays filled with 0xFF.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "k4_facade_test_util.h"

struct Case {
  int form, rhamm, both, klen, nth, iib;
  uint32_t mn, mx, entry, loci, len;
  std::vector<etSeqBase> seq;
  std::vector<uint8_t> want;
};

static int RunCase(CSfxArray* pSfx, const Case& c) {
  std::vector<uint8_t> Out(c.len + 4, 0xff);
  std::vector<etSeqBase> Seq = c.seq;
  Seq.resize(Seq.size() + 8);
  const int Rslt = c.form == 0 ? pSfx->LocateSfxHammings(c.rhamm, c.both != 0, c.klen, c.nth, (int)c.len, c.mn, c.mx, c.entry, c.loci, c.iib, Out.data(), 0, nullptr)
                               : pSfx->LocateHammings(c.rhamm, c.both != 0, c.klen, c.nth, (int)c.len, c.mn, c.mx, Seq.data(), 0, 0, c.iib, Out.data(), 0, nullptr);
  if (Rslt != 0) return -1;
  if (memcmp(Out.data(), c.want.data(), c.len) != 0) return -2;
  for (size_t k = c.len; k < Out.size(); k++)
    if (Out[k] != 0xff) return -3;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  CSfxArray* pSfx = new CSfxArray;
  if (const int rc = K4FtOpen(pSfx, argv[1])) return rc;
  FILE* f = fopen(argv[2], "r");
  if (!f) return 4;
  std::vector<Case> Cases;
  for (;;) {
    Case c;
    if (fscanf(f, "%d %d %d %d %d %u %u %d %u %u %u", &c.form, &c.rhamm, &c.both, &c.klen, &c.nth, &c.mn, &c.mx, &c.iib, &c.entry, &c.loci, &c.len) != 11) break;
    if (c.form == 1 && !K4FtReadProbe(f, c.len, c.seq)) return 5;
    for (uint32_t k = 0; k < c.len; k++) {
      unsigned v;
      if (fscanf(f, "%u", &v) != 1) return 5;
      c.want.push_back((uint8_t)v);
    }
    Cases.push_back(c);
  }
  fclose(f);
  const int NT = 8;
  std::vector<int> Bad(NT, 0);
  auto Work = [&](int t) {
    for (size_t i = 0; i < Cases.size(); i++) {
      const size_t q = (i + (size_t)t * 7) % Cases.size();  // (the threads are at different spans at any one time)
      if (RunCase(pSfx, Cases[q]) != 0) Bad[(size_t)t]++;
    }
  };
  std::vector<std::thread> Th;
  for (int t = 0; t < NT; t++) Th.emplace_back(Work, t);
  for (auto& t : Th) t.join();
  int bad = 0;
  for (int t = 0; t < NT; t++) bad += Bad[(size_t)t];
  printf("threads %d cases %zu bad %d msgs %d\n", NT, Cases.size(), bad, pSfx->NumErrMsgs());
  uint8_t One[64];
  memset(One, 0xff, sizeof(One));
  printf("entry 0 -> %d\n", pSfx->LocateSfxHammings(3, false, 60, 1, 60, 3, 4, 0, 0, 0, One));
  printf("short span -> %d\n", pSfx->LocateSfxHammings(3, false, 60, 1, 59, 3, 4, 1, 0, 0, One));
  printf("past entry -> %d\n", pSfx->LocateSfxHammings(3, false, 60, 1, 60, 3, 4, 1, pSfx->GetSeqLen(1) - 59, 0, One));
  const int Narrow = pSfx->LocateSfxHammings(10, false, 60, 1, 60, 3, 4, 1, 0, 0, One);
  printf("core under 8 -> %d msgs %d\n", Narrow, pSfx->NumErrMsgs());
  printf("untouched %d\n", One[0] == 0xff ? 1 : 0);
  delete pSfx;
  return 0;
}
