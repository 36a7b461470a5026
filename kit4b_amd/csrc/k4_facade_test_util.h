// kit4b_amd/csrc/k4_facade_test_util.h -- what the k4_*facade_test programs start with: the index opened the way the reference's
// front ends open theirs, and the probes of their case files, which are written as one word of etSeqBase digits.
#pragma once
#include <cstdio>
#include <vector>
#include "k4_sfxarray.hpp"

// Open and SetTargBlock(1).  0, or the program's exit code: 2 with the facade's messages on stderr, 3.
static inline int K4FtOpen(CSfxArray* pSfx, char* pszSfxFile) {
  if (pSfx->Open(pszSfxFile) < 0) {
    while (pSfx->NumErrMsgs()) fprintf(stderr, "%s\n", pSfx->GetErrMsg());
    return 2;
  }
  return pSfx->SetTargBlock(1) < 0 ? 3 : 0;
}

// the first len digits of a word as bases
static inline void K4FtDigits(const char* pszWord, unsigned len, etSeqBase* pSeq) {
  for (unsigned j = 0; j < len; j++) pSeq[j] = (etSeqBase)(pszWord[j] - '0');
}

// the next word of f as a probe of len bases ("-" stands for none), with pad zero bases behind them; false at the end of the file
static inline bool K4FtReadProbe(FILE* f, unsigned len, std::vector<etSeqBase>& Seq, unsigned pad = 0) {
  std::vector<char> s(len + 2);
  if (fscanf(f, "%s", s.data()) != 1) return false;
  Seq.assign(len + pad, 0);
  K4FtDigits(s.data(), len, Seq.data());
  return true;
}
