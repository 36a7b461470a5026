// include/k4_sfxarray.hpp -- C++ facade that keeps the CSfxArray call surface CKAligner uses
// (libkit4b/SfxArray.h:524-1023; call sites: `grep m_pSfxArray-> ngskit4b/KAligner.cpp`) on top of the C ABI of
// libk4sfx.so (include/k4sfx.h).  Header-only, plain C++11, no HIP / torch types.
//
// Same names, argument meaning, ownership and error behaviour as the reference:
//   * results < 0 are teBSFrsltCodes, 0..4 tHRslt; text is queued and drained with NumErrMsgs()/GetErrMsg()
//   * the caller owns the probe buffer (left unchanged), pHits[MaxHits] and the ident-node scratch (accepted and ignored:
//     the GPU path keeps its own dedupe state)
//   * AlignReads() forwards one read as a batch of 1; throughput callers use AlignReadsBatch() / KAlignBatch()
#ifndef K4_SFXARRAY_HPP
#define K4_SFXARRAY_HPP
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <vector>
#include "k4sfx.h"

#ifndef K4_HAVE_KIT4B_TYPES  // (define it when libkit4b's own headers already provide these types)
typedef uint8_t etSeqBase;  // libkit4b/commdefs.h:87
enum { eBaseA = 0, eBaseC, eBaseG, eBaseT, eBaseN, eBaseUndef, eBaseInDel, eBaseEOS };

typedef enum etALStrand { eALSboth, eALSWatson, eALSCrick, eALSnone } eALStrand;                 // SfxArray.h:72-77
typedef enum etHRslt { eHRnone = 0, eHRhits, eHRMMDelta, eHRHitInsts, eHRRMMDelta, eHRSeqErrs, eHRFatalError } tHRslt;  // :79-87

#pragma pack(1)
typedef struct TAG_sSegLoci {  // libkit4b/SfxArray.h:239-249 (23 bytes)
  uint16_t ReadOfs;
  uint8_t Strand;
  uint32_t ChromID;
  uint64_t MatchLoci;
  uint16_t MatchLen;
  uint8_t Mismatches;
  uint16_t TrimLeft;
  uint16_t TrimRight;
  uint8_t TrimMismatches;
} tsSegLoci;
typedef struct TAG_tsHitLoci {  // libkit4b/SfxArray.h:251-260 (50 bytes)
  etSeqBase BisBase;
  uint8_t FlgChimeric : 1;
  uint8_t FlgInDel : 1;
  uint8_t FlgInsert : 1;
  uint8_t FlgSplice : 1;
  uint8_t FlgNonOrphan : 1;
  uint16_t Score;
  tsSegLoci Seg[2];
} tsHitLoci;
#pragma pack()
#pragma pack(4)
typedef struct TAG_sSfxHeaderV3 {  // libkit4b/SfxArray.h:194-207 (1224 bytes)
  uint8_t Magic[4];
  int32_t Version;
  uint32_t Attributes;
  uint64_t FileLen;
  uint64_t EntriesOfs;
  uint32_t EntriesSize;
  uint32_t NumSfxBlocks;
  uint64_t SfxBlockSize;
  uint64_t SfxBlockOfs;
  uint8_t szDatasetName[81];
  uint8_t szDescription[1024];
  uint8_t szTitle[64];
} tsSfxHeaderV3;
#pragma pack()
typedef struct TAG_sIdentNode {  // libkit4b/SfxArray.h:144-147 (caller scratch; unused here)
  uint32_t TargSeqID;
  struct TAG_sIdentNode* pNxt;
} tsIdentNode;
#pragma pack(1)
typedef struct TAG_sQueryAlignNodes {  // libkit4b/SfxArray.h:149-165 (41 bytes)
  uint32_t AlignNodeID;
  uint8_t FlgStrand : 1;
  uint8_t FlgFirst2tRpt : 1;
  uint8_t Flg2Rpt : 1;
  uint8_t FlgScored : 1;
  uint8_t FlgRedundant : 1;
  int32_t QueryID;
  uint32_t QueryStartOfs;
  uint32_t AlignLen;
  uint32_t TargSeqID;
  uint32_t TargSeqLoci;
  uint32_t NumMismatches;
  int32_t HiScore;
  uint32_t HiScorePathNextIdx;
  uint32_t NxtHashMatch;
} tsQueryAlignNodes;
#pragma pack()
const int cMaxCultivars = 20000;         // libkit4b/SfxArray.h:186-189
const int cMinCultivarPreSufLen = 5;
const int cMaxCultivarPreSufLen = 200;
const int cTotCultivarKMerLen = 300;
#pragma pack(1)                     // (libkit4b/SfxArray.h:227-320 is one pack(1) region)
typedef struct TAG_sKMerCultCnts {  // libkit4b/SfxArray.h:262-266
  uint32_t EntryID;
  uint32_t SenseCnts;
  uint32_t AntisenseCnts;
} tsKMerCultDist;
typedef struct TAG_sKMerCultsCnts {  // libkit4b/SfxArray.h:268-275
  uint64_t SenseCnts;
  uint64_t AntisenseCnts;
  uint32_t NumCultivars;
  uint32_t TotCultivars;
  etSeqBase KMerSeq[cTotCultivarKMerLen + 1];
  tsKMerCultDist CultCnts[cMaxCultivars];
} tsKMerCultsCnts;
#pragma pack()
#endif  // K4_HAVE_KIT4B_TYPES
static_assert(sizeof(tsKMerCultDist) == 12 && sizeof(tsKMerCultsCnts) == 240325 && offsetof(tsKMerCultsCnts, CultCnts) == 325 &&
                  offsetof(tsKMerCultsCnts, KMerSeq) == 24,
              "layouts must match libkit4b");
static_assert(sizeof(tsSegLoci) == 23 && sizeof(tsHitLoci) == 50 && sizeof(tsSfxHeaderV3) == 1224, "layouts must match libkit4b");
static_assert(sizeof(tsQueryAlignNodes) == 41, "layouts must match libkit4b");

class CSfxArray {
  k4_index* m_pIdx;
  int m_Device;
  int m_MaxIter;
  std::deque<std::string> m_Errs;
  std::mutex m_Mtx;  // CKAligner calls AlignReads / AlignPairedRead from many threads on one object; an
                     // index handle runs one batch at a time: whoever talks to the device holds this
  // AlignReads calls that arrive while a batch is on the device are collected and go out together as the next batch: the
  // first caller to find no batch in flight becomes the leader, runs the pending requests (grouped by parameter set) and
  // wakes their owners; with T caller threads the device sees batches of up to T reads instead of T batches of one.
  struct Req {
    k4_align_params p;
    const etSeqBase* probe;
    uint32_t len;
    int32_t rslt, inst, low, nxt, rc;
    std::vector<k4_hit> hits;
    k4_seg2 seg2;  // the second segment of a microInDel / splice-junction hit (slot 0)
    bool done;
    // a LocateQuerySeqs call travels the same way: qp instead of p, nodes instead of hits
    bool query = false;
    k4_query_params qp;
    std::vector<k4_query_node> nodes;
  };
  std::mutex m_QMtx;
  std::condition_variable m_QCv;
  std::vector<Req*> m_Pending;
  bool m_LeaderActive = false;

  void RunQueryGroup(std::vector<Req*>& g) {  // same parameters: one k4_locate_query_seqs_batch
    const size_t n = g.size();
    std::vector<uint8_t> cat;
    std::vector<uint64_t> offs(n), node_offs(n + 1, 0);
    std::vector<uint32_t> lens(n);
    for (size_t i = 0; i < n; i++) {
      offs[i] = cat.size();
      lens[i] = g[i]->len;
      cat.insert(cat.end(), g[i]->probe, g[i]->probe + g[i]->len);
    }
    cat.resize(cat.size() + 16);
    std::vector<k4_query_node> nodes(n * (size_t)g[0]->qp.max_hits);  // (a query returns at most max_hits nodes)
    int rc;
    {
      std::lock_guard<std::mutex> dev(m_Mtx);
      rc = k4_locate_query_seqs_batch(m_pIdx, &g[0]->qp, (int64_t)n, cat.data(), offs.data(), lens.data(), node_offs.data(), nodes.data(),
                                      (uint64_t)nodes.size());
      if (rc != K4_OK) Fail(rc);
    }
    for (size_t i = 0; i < n; i++) {
      g[i]->rc = rc;
      if (rc == K4_OK) g[i]->nodes.assign(nodes.begin() + (ptrdiff_t)node_offs[i], nodes.begin() + (ptrdiff_t)node_offs[i + 1]);
    }
  }
  void RunGroup(std::vector<Req*>& g) {  // same parameters: one k4_align_reads_batch
    if (g[0]->query) { RunQueryGroup(g); return; }
    const size_t n = g.size();
    std::vector<uint8_t> cat;
    std::vector<uint64_t> offs(n);
    std::vector<uint32_t> lens(n);
    for (size_t i = 0; i < n; i++) {
      offs[i] = cat.size();
      lens[i] = g[i]->len;
      cat.insert(cat.end(), g[i]->probe, g[i]->probe + g[i]->len);
    }
    cat.resize(cat.size() + 16);
    const int mh = g[0]->p.max_hits;
    std::vector<int32_t> r(4 * n);
    std::vector<k4_hit> h(n * (size_t)mh);
    std::vector<k4_seg2> s2(n);
    int rc;
    {
      std::lock_guard<std::mutex> dev(m_Mtx);
      rc = k4_align_reads_ext_batch(m_pIdx, &g[0]->p, (int64_t)n, cat.data(), offs.data(), lens.data(), r.data(), r.data() + n,
                                    r.data() + 2 * n, r.data() + 3 * n, h.data(), s2.data());
      if (rc != K4_OK) Fail(rc);
    }
    for (size_t i = 0; i < n; i++) {
      Req* q = g[i];
      q->seg2 = s2[i];
      q->rc = rc; q->rslt = r[i]; q->inst = r[n + i]; q->low = r[2 * n + i]; q->nxt = r[3 * n + i];
      q->hits.assign(h.begin() + (ptrdiff_t)(i * mh), h.begin() + (ptrdiff_t)((i + 1) * mh));
    }
  }
  void Submit(Req& rq) {
    std::unique_lock<std::mutex> lk(m_QMtx);
    m_Pending.push_back(&rq);
    while (!rq.done) {
      if (m_LeaderActive) {  // a batch is on the device: this request goes with the next one
        m_QCv.wait(lk);
        continue;
      }
      m_LeaderActive = true;  // lead one batch: everything pending right now, this request included
      std::vector<Req*> batch;
      batch.swap(m_Pending);
      lk.unlock();
      std::vector<char> taken(batch.size(), 0);
      for (size_t i = 0; i < batch.size(); i++) {
        if (taken[i]) continue;
        std::vector<Req*> g;
        for (size_t j = i; j < batch.size(); j++)
          if (!taken[j] && batch[j]->query == batch[i]->query &&
              (batch[i]->query ? std::memcmp(&batch[j]->qp, &batch[i]->qp, sizeof(k4_query_params))
                               : std::memcmp(&batch[j]->p, &batch[i]->p, sizeof(k4_align_params))) == 0) {
            g.push_back(batch[j]);
            taken[j] = 1;
          }
        RunGroup(g);
      }
      lk.lock();
      for (Req* q : batch) q->done = true;
      m_LeaderActive = false;
      m_QCv.notify_all();
    }
  }

  int m_OccKMerLen = 0, m_MaxKMerOccs = 0;  // InitOverOccKMers
  std::vector<uint16_t> m_IdentFlags;  // per entry, the flags half of tsSfxEntry.fBlockID (SfxArray.cpp:2048-2079)

  bool LoadIdentFlags() {
    if (!m_pIdx) return false;
    if (m_IdentFlags.empty()) {
      const int n = GetNumEntries();
      m_IdentFlags.resize((size_t)n, 0);
      for (int e = 1; e <= n; e++) {
        k4_entry ent;
        if (k4_get_entry(m_pIdx, (uint32_t)e, &ent) == K4_OK) m_IdentFlags[(size_t)e - 1] = (uint16_t)((ent.fblock_id >> 8) & 0xffff);
      }
    }
    return true;
  }

  int Fail(int rc) {
    const char* m = m_pIdx ? k4_last_error(m_pIdx) : k4_global_error();
    m_Errs.push_back(m ? m : "");
    return rc;
  }
  // n symbols of the concatenation from offset psn, for GenKMerCultThreadRange: what lies behind the end of psn's sequence reads as
  // `fill`, a code that is no base
  void ConcatBases(uint64_t psn, int n, etSeqBase fill, std::vector<etSeqBase>& out) {
    out.assign((size_t)n, fill);
    k4_info_t inf;
    if (k4_info(m_pIdx, &inf) != K4_OK) return;
    uint32_t lo = 1, hi = inf.n_entries;
    while (lo <= hi) {  // (the table is sorted by start_ofs, entry ids 1..n in that order)
      const uint32_t mid = (lo + hi) / 2;
      k4_entry e;
      if (k4_get_entry(m_pIdx, mid, &e) != K4_OK) return;
      if (e.start_ofs > psn) hi = mid - 1;
      else if (e.start_ofs + e.seq_len <= psn) lo = mid + 1;
      else { k4_get_seq(m_pIdx, mid, (uint32_t)(psn - e.start_ofs), out.data(), (uint32_t)n); return; }
    }
  }
  // the flat records -> tsHitLoci as LocateCoreMultiples (SfxArray.cpp:6264-6307, chimeric :6123-6146), LocateInDels
  // (:7800-7825) and LocateSpliceJuncts (:7501-7516) leave it
  static void Expand(const k4_hit& h, tsHitLoci* p, const k4_seg2* s2 = nullptr) {
    std::memset(p, 0, sizeof(*p));
    p->BisBase = eBaseN;
    p->FlgChimeric = (h.ext & K4_EXT_CHIMERIC) ? 1 : 0;
    p->FlgInDel = (h.ext & K4_EXT_INDEL) ? 1 : 0;
    p->FlgInsert = (h.ext & K4_EXT_INSERT) ? 1 : 0;
    p->FlgSplice = (h.ext & K4_EXT_SPLICE) ? 1 : 0;
    p->FlgNonOrphan = (h.ext & K4_EXT_NONORPHAN) ? 1 : 0;
    p->Seg[0].Strand = h.strand;
    p->Seg[0].ChromID = h.chrom_id;
    p->Seg[0].MatchLoci = h.match_loci;
    p->Seg[0].MatchLen = h.match_len;
    p->Seg[0].Mismatches = h.mismatches;
    p->Seg[0].TrimMismatches = h.mismatches;
    p->Seg[0].TrimLeft = (uint16_t)K4_HIT_TRIM_LEFT(h);
    p->Seg[0].TrimRight = (uint16_t)K4_HIT_TRIM_RIGHT(h);
    if (s2 && (h.ext & (K4_EXT_INDEL | K4_EXT_SPLICE))) {
      p->Score = s2->score;
      p->Seg[1].ReadOfs = s2->read_ofs;
      p->Seg[1].Strand = h.strand;
      p->Seg[1].ChromID = s2->chrom_id;
      p->Seg[1].MatchLoci = s2->match_loci;
      p->Seg[1].MatchLen = s2->match_len;
      p->Seg[1].Mismatches = s2->mismatches;
      p->Seg[1].TrimMismatches = s2->mismatches;
    }
  }

 public:
  explicit CSfxArray(int Device = 0) : m_pIdx(nullptr), m_Device(Device), m_MaxIter(50000) {}
  ~CSfxArray() { Reset(); }
  CSfxArray(const CSfxArray&) = delete;
  CSfxArray& operator=(const CSfxArray&) = delete;

  int Reset(bool bFlush = true) {  // SfxArray.h:527
    (void)bFlush;
    if (m_pIdx) k4_close(m_pIdx);
    m_pIdx = nullptr;
    m_IdentFlags.clear();
    return 0;
  }
  int Close(bool bFlush = true) { return Reset(bFlush); }  // SfxArray.h:548

  // Open an existing .sfx (creation goes through `ngskit4b index` or k4_build_sa_device + k4_write_sfx).  SfxArray.h:528
  int Open(char* pszSeqFile, bool bCreate = false, bool bBisulfite = false, bool bColorspace = false) {
    Reset();
    if (bCreate || bBisulfite || bColorspace) {
      m_Errs.push_back("CSfxArray::Open: create/bisulfite/colorspace are outside the accelerated path");
      return K4_ERR_UNSUPPORTED;
    }
    int rc = k4_open(pszSeqFile, m_Device, 0, &m_pIdx);
    if (rc != K4_OK) return Fail(rc);
    k4_set_max_iter(m_pIdx, m_MaxIter);
    return 0;
  }
  int SetTargBlock(int BlockID) { return (m_pIdx && BlockID == 1) ? 0 : K4_ERR_PARAMS; }  // SfxArray.h:957: index already resident
  int Next(int PrevBlockID = 0) { return PrevBlockID == 0 && m_pIdx ? 1 : 0; }
  int SetMaxIter(int MaxIter) {  // SfxArray.h:556
    int prev = m_MaxIter;
    m_MaxIter = MaxIter > 0 ? MaxIter : 0;
    if (m_pIdx) k4_set_max_iter(m_pIdx, m_MaxIter);
    return prev;
  }
  int GetMaxIter(void) { return m_MaxIter; }
  int InitialiseCoreKMers(int KMerLen) { (void)KMerLen; return m_pIdx ? 0 : K4_ERR_INTERNAL; }  // SfxArray.h:1017: the k-mer table replaces the memo
  bool IsSOLiD(void) { return false; }

  int GetNumEntries(void) {  // SfxArray.h:958
    k4_info_t i;
    return m_pIdx && k4_info(m_pIdx, &i) == K4_OK ? (int)i.n_entries : 0;
  }
  uint64_t GetTotSeqsLen(void) {  // SfxArray.h:970
    k4_info_t i;
    return m_pIdx && k4_info(m_pIdx, &i) == K4_OK ? i.tot_seqs_len : 0;
  }
  uint32_t GetSeqLen(uint32_t EntryID) {  // SfxArray.h:969
    k4_entry e;
    return m_pIdx && k4_get_entry(m_pIdx, EntryID, &e) == K4_OK ? e.seq_len : 0;
  }
  int GetIdentName(uint32_t EntryID, int MaxLen, char* pszSeqIdent) {  // SfxArray.h:967
    k4_entry e;
    if (!m_pIdx || !pszSeqIdent || MaxLen < 1 || k4_get_entry(m_pIdx, EntryID, &e) != K4_OK) return K4_ERR_ENTRY;
    std::strncpy(pszSeqIdent, e.name, (size_t)MaxLen);
    pszSeqIdent[MaxLen - 1] = '\0';
    return 0;
  }
  int GetIdent(char* pszSeqIdent) { return m_pIdx ? k4_get_ident(m_pIdx, pszSeqIdent) : K4_ERR_ENTRY; }  // SfxArray.h:968
  char* GetDatasetName(void) {
    static thread_local char name[81];
    k4_info_t i;
    name[0] = 0;
    if (m_pIdx && k4_info(m_pIdx, &i) == K4_OK) std::strncpy(name, i.dataset, 80);
    return name;
  }
  uint32_t GetSeq(int EntryID, uint32_t Loci, etSeqBase* pRetSeq, uint32_t Len) {  // SfxArray.h:996
    std::lock_guard<std::mutex> lock(m_Mtx);
    return m_pIdx ? (uint32_t)k4_get_seq(m_pIdx, (uint32_t)EntryID, Loci, pRetSeq, Len) : 0;
  }
  int GetBase(int EntryID, uint32_t Loci) {  // SfxArray.h:992
    etSeqBase b;
    return GetSeq(EntryID, Loci, &b, 1) == 1 ? (int)b : K4_ERR_PARAMS;
  }
  int NumErrMsgs(void) { return (int)m_Errs.size(); }  // CErrorCodes, ErrorCodes.h:99-113
  char* GetErrMsg(void) {
    static thread_local std::string cur;
    if (m_Errs.empty()) return (char*)"";
    cur = m_Errs.front();
    m_Errs.pop_front();
    return (char*)cur.c_str();
  }
  k4_index* Handle(void) { return m_pIdx; }

  // per-entry flags (SfxArray.h:959-965): kept on the host, they never reach the device
  void InitAllIdentFlags(uint16_t Flags = 0) {
    if (LoadIdentFlags()) std::fill(m_IdentFlags.begin(), m_IdentFlags.end(), Flags);
  }
  uint16_t GetIdentFlags(uint32_t EntryID) {
    if (!LoadIdentFlags() || EntryID < 1 || EntryID > m_IdentFlags.size()) return (uint16_t)K4_ERR_ENTRY;
    return m_IdentFlags[EntryID - 1];
  }
  uint16_t SetResetIdentFlags(uint32_t EntryID, uint16_t SetFlags = 0, uint16_t ResetFlags = 0) {  // returns the flags before the call
    if (SetFlags == 0 && ResetFlags == 0) return GetIdentFlags(EntryID);
    if (!LoadIdentFlags() || EntryID < 1 || EntryID > m_IdentFlags.size()) return (uint16_t)K4_ERR_ENTRY;
    const uint16_t prev = m_IdentFlags[EntryID - 1];
    m_IdentFlags[EntryID - 1] = (uint16_t)((prev | SetFlags) & ~ResetFlags);
    return prev;
  }
  int GetSfxHeader(tsSfxHeaderV3* pSfxHeader) {  // SfxArray.h:551
    if (!m_pIdx || !pSfxHeader) return K4_ERR_PARAMS;
    return k4_get_sfx_header(m_pIdx, pSfxHeader);
  }
  int GetColorspaceSeq(int EntryID, uint32_t Loci, etSeqBase* pRetSeq, uint32_t Len) {  // SOLiD only; IsSOLiD() is false here
    (void)EntryID; (void)Loci; (void)pRetSeq; (void)Len;
    m_Errs.push_back("CSfxArray::GetColorspaceSeq: colourspace indexes are outside the accelerated path");
    return K4_ERR_UNSUPPORTED;
  }

  // CSfxArray::AlignReads, SfxArray.h:614-634 -- identical parameter list.
  int AlignReads(uint32_t ExtdProcFlags, uint32_t ReadID, int MinChimericLen, int TotMM, int CoreLen, int CoreDelta,
                 int MaxNumCoreSlides, int MinCoreLen, int MMDelta, eALStrand Align2Strand, int microInDelLen,
                 int MaxSpliceJunctLen, int* pLowHitInstances, int* pLowMMCnt, int* pNxtLowMMCnt, etSeqBase* pProbeSeq,
                 int ProbeLen, int MaxHits, tsHitLoci* pHits, int NumAllocdIdentNodes, tsIdentNode* pAllocsIdentNodes) {
    (void)ExtdProcFlags; (void)ReadID; (void)NumAllocdIdentNodes; (void)pAllocsIdentNodes;
    if (!m_pIdx) return K4_ERR_INTERNAL;
    if (*pLowHitInstances > 0) {  // carried-in hits (never passed by CKAligner::AlignRead, KAligner.cpp:9609-9611)
      m_Errs.push_back("CSfxArray::AlignReads: carried-in LowHitInstances > 0 is not supported");
      return K4_ERR_UNSUPPORTED;
    }
    if (Align2Strand == eALSnone) return eHRnone;
    if (ProbeLen < 1 || MaxHits < 1) return K4_ERR_PARAMS;
    Req rq;
    // MinChimericLen outside 15..99 means "no trimming" to LocateCoreMultiples (:5878-5883) but still runs its extra pass
    rq.p = k4_align_params{TotMM, CoreLen, CoreDelta, MaxNumCoreSlides, MinCoreLen, MMDelta, (int32_t)Align2Strand, MaxHits,
                           MinChimericLen > 0 ? MinChimericLen : 0, microInDelLen > 0 ? microInDelLen : 0,
                           MaxSpliceJunctLen > 0 ? MaxSpliceJunctLen : 0};
    std::memset(&rq.seg2, 0, sizeof(rq.seg2));
    rq.probe = pProbeSeq; rq.len = (uint32_t)ProbeLen;
    rq.rslt = rq.inst = rq.low = rq.nxt = 0; rq.rc = K4_OK; rq.done = false;
    Submit(rq);  // alone: a batch of one; with other threads calling at the same time: one batch for all of them
    if (rq.rc != K4_OK) return rq.rc;
    *pLowHitInstances = rq.inst; *pLowMMCnt = rq.low; *pNxtLowMMCnt = rq.nxt;
    int nvalid = (rq.rslt >= eHRhits && rq.rslt <= eHRHitInsts) ? (rq.inst < MaxHits ? rq.inst : MaxHits) : 0;
    for (int i = 0; i < nvalid; i++) Expand(rq.hits[(size_t)i], &pHits[i], i == 0 ? &rq.seg2 : nullptr);
    return rq.rslt;
  }

  // CSfxArray::LocateBestMatches, SfxArray.h:793-806 -- identical parameter list (CKAligner's -N, KAligner.cpp:9779).
  // Returns 0 (no match), 1..MaxHits, or MaxHits+1 when further matches were sloughed.
  int LocateBestMatches(uint32_t ReadID, int MaxTotMM, int CoreLen, int CoreDelta, int MaxNumCoreSlides, eALStrand Align2Strand,
                        etSeqBase* pProbeSeq, int ProbeLen, int MaxHits, int* pHitInstances, tsHitLoci* pHits, int CurMaxIter,
                        int NumAllocdIdentNodes, tsIdentNode* pAllocsIdentNodes) {
    (void)ReadID; (void)NumAllocdIdentNodes; (void)pAllocsIdentNodes;
    if (!m_pIdx) return K4_ERR_INTERNAL;
    if (pHitInstances) *pHitInstances = 0;
    if (Align2Strand == eALSnone) return 0;
    std::lock_guard<std::mutex> lock(m_Mtx);
    const int prev_iter = CurMaxIter != m_MaxIter ? k4_set_max_iter(m_pIdx, CurMaxIter) : -1;
    k4_align_params p = {MaxTotMM, CoreLen, CoreDelta, MaxNumCoreSlides, 0, 1, (int32_t)Align2Strand, MaxHits};
    uint64_t off = 0;
    uint32_t len = (uint32_t)ProbeLen;
    int32_t rslt = 0, inst = 0;
    std::vector<k4_hit> hits((size_t)MaxHits);
    int rc = k4_best_matches_batch(m_pIdx, &p, 1, pProbeSeq, &off, &len, &rslt, &inst, hits.data());
    if (prev_iter >= 0) k4_set_max_iter(m_pIdx, prev_iter);
    if (rc != K4_OK) return Fail(rc);
    if (pHitInstances) *pHitInstances = inst;
    for (int i = 0; i < inst && i < MaxHits; i++) Expand(hits[(size_t)i], &pHits[i]);
    return rslt;
  }

  // CSfxArray::InitOverOccKMers, SfxArray.h:559-561.  The reference caches, per k-mer of KMerLen bases, whether it occurs 0,
  // 1..MaxKMerOccs or more times, and LocateQuerySeqs skips a core of that length unless it is in the middle class.  Here no
  // cache is built: for such calls the depth becomes min(CurMaxIter, MaxKMerOccs + 1), which skips the same ACGT cores.  A core
  // that holds N is counted as it is (the reference's cache indexes N as A, and what it answers depends on which thread
  // touched the k-mer first).
  int InitOverOccKMers(int KMerLen, int MaxKMerOccs) {
    if (!m_pIdx) return K4_ERR_INTERNAL;
    if (KMerLen < 1 || MaxKMerOccs < 1) { m_OccKMerLen = m_MaxKMerOccs = 0; return K4_ERR_PARAMS; }
    m_OccKMerLen = KMerLen; m_MaxKMerOccs = MaxKMerOccs;
    return 0;
  }

  // CSfxArray::LocateQuerySeqs, SfxArray.h:779-790 -- identical parameter list (CBlitz's engine call, Blitz.cpp).  Returns the
  // number of nodes left in pHits[0 ..]; AlignNodeID, QueryID and the cleared flags / scores as the reference leaves them,
  // NxtHashMatch 0 (the reference leaves the chain links of before its compaction there).  Concurrent calls share a device batch.
  int LocateQuerySeqs(uint32_t QuerySeqID, etSeqBase* pProbeSeq, uint32_t ProbeLen, uint32_t CoreLen, uint32_t CoreDelta,
                      eALStrand Align2Strand, uint32_t MaxHits, tsQueryAlignNodes* pHits, uint32_t CurMaxIter, int BaseMatchPts,
                      int BaseMismatchPts) {
    if (!m_pIdx) return K4_ERR_INTERNAL;
    if (!pProbeSeq || !pHits || MaxHits > 0x7fffffffu || CoreLen > 0x7fffffffu || CoreDelta > 0x7fffffffu) return K4_ERR_PARAMS;
    uint32_t Depth = CurMaxIter > 0x7fffffffu ? 0x7fffffffu : CurMaxIter;
    if (m_OccKMerLen > 0 && CoreLen == (uint32_t)m_OccKMerLen && Depth > (uint32_t)m_MaxKMerOccs + 1) Depth = (uint32_t)m_MaxKMerOccs + 1;
    Req rq;
    std::memset(&rq.p, 0, sizeof(rq.p));
    std::memset(&rq.seg2, 0, sizeof(rq.seg2));
    rq.query = true;
    rq.qp = k4_query_params{(int32_t)CoreLen, (int32_t)CoreDelta, (int32_t)Align2Strand, (int32_t)MaxHits, (int32_t)Depth, BaseMatchPts,
                            BaseMismatchPts};
    rq.probe = pProbeSeq; rq.len = ProbeLen;
    rq.rslt = rq.inst = rq.low = rq.nxt = 0; rq.rc = K4_OK; rq.done = false;
    Submit(rq);
    if (rq.rc != K4_OK) return rq.rc;
    for (size_t i = 0; i < rq.nodes.size(); i++) {
      const k4_query_node& n = rq.nodes[i];
      tsQueryAlignNodes* h = &pHits[i];
      std::memset(h, 0, sizeof(*h));  // the flags, HiScore, HiScorePathNextIdx, NxtHashMatch
      h->AlignNodeID = n.slot;
      h->FlgStrand = n.strand ? 1 : 0;
      h->QueryID = (int32_t)QuerySeqID;
      h->QueryStartOfs = n.query_start; h->AlignLen = n.align_len;
      h->TargSeqID = n.targ_seq_id; h->TargSeqLoci = n.targ_loci; h->NumMismatches = n.n_mismatches;
    }
    return (int)rq.nodes.size();
  }

  // CSfxArray::GenKMerCultThreadRange, SfxArray.cpp:2733-2801, on the host from the few elements and bases it looks at.  As there,
  // the inclusive end it returns is the first element of the NEXT K-mer, so a K-mer that straddles two ranges is located by both.
  int GenKMerCultThreadRange(int KMerLen, int ThreadInst, int NumThreads, int64_t StartSfxIdx, int64_t* pEndSfxIdx) {
    if (NumThreads < 1 || NumThreads > 64 || ThreadInst < 1 || ThreadInst > NumThreads || StartSfxIdx < 0 || pEndSfxIdx == nullptr) return -1;
    *pEndSfxIdx = 0;
    k4_info_t inf;
    if (!m_pIdx || k4_info(m_pIdx, &inf) != K4_OK) return -1;
    const int64_t NumSfxEls = (int64_t)inf.concat_len;
    if (StartSfxIdx >= NumSfxEls) return -1;
    if ((NumSfxEls - StartSfxIdx) < 50000) { *pEndSfxIdx = NumSfxEls - 1; return 1; }
    int64_t PutativeEndSfxEl = StartSfxIdx + (NumSfxEls - StartSfxIdx) / (1 + NumThreads - ThreadInst);
    if ((PutativeEndSfxEl + 25000) >= NumSfxEls) { *pEndSfxIdx = NumSfxEls - 1; return 1; }
    std::lock_guard<std::mutex> lk(m_Mtx);
    std::vector<etSeqBase> El1, El2;
    uint64_t TargPsn1 = 0, TargPsn2 = 0;
    if (k4_get_sfx_els(m_pIdx, (uint64_t)PutativeEndSfxEl, 1, &TargPsn1) != K4_OK) return -1;
    ConcatBases(TargPsn1, KMerLen, 0x0f, El1);
    for (PutativeEndSfxEl += 1; PutativeEndSfxEl < NumSfxEls; PutativeEndSfxEl++) {
      if (k4_get_sfx_els(m_pIdx, (uint64_t)PutativeEndSfxEl, 1, &TargPsn2) != K4_OK) return -1;
      if ((int64_t)TargPsn2 + KMerLen >= NumSfxEls) { *pEndSfxIdx = PutativeEndSfxEl; return 1; }
      ConcatBases(TargPsn2, KMerLen, 0x0e, El2);
      for (int Ofs = 0; Ofs < KMerLen; Ofs++)
        if ((El1[Ofs] & 0x0f) > eBaseT || (El1[Ofs] & 0x0f) != (El2[Ofs] & 0x0f)) { *pEndSfxIdx = PutativeEndSfxEl; return 1; }
    }
    return 0;
  }

  // CSfxArray::GenKMerCultsCnts, SfxArray.cpp:2804-3079 -- identical parameter list (`ngskit4b kmermarkers`, MarkerKMers.cpp:874).
  // The resumable device call is repeated; every reported K-mer is rebuilt as the dense tsKMerCultsCnts the reference hands over
  // (TotCultivars entries with EntryID = place + 1, zero elsewhere), held on the heap, and only the entries a K-mer touched are
  // cleared for the next.  A callback result below 0 ends the call with that value.  MaxHomozygotic > 0 with a suffix is not
  // built (K4_ERR_UNSUPPORTED, with a message); without a suffix it is ignored as the reference ignores it.
  int64_t GenKMerCultsCnts(bool bSenseOnly, int64_t StartSfxIdx, int64_t EndSfxIdx, int PrefixKMerLen, int SuffixKMerLen, int MinCultivars,
                           int MaxHomozygotic, void* pThis, int (*pCallback)(void* pThis, tsKMerCultsCnts* pCultsCnts)) {
    if (!m_pIdx || !pCallback) return -1;
    k4_info_t inf;
    if (k4_info(m_pIdx, &inf) != K4_OK) return -1;
    const k4_cults_params p = {PrefixKMerLen, SuffixKMerLen, MinCultivars, bSenseOnly ? 1 : 0, 0, MaxHomozygotic};
    const uint64_t max_kmers = 1u << 16, max_dist = std::max<uint64_t>(inf.n_entries, 8 * max_kmers);  // (a call's windows follow its room)
    const int klen = PrefixKMerLen + SuffixKMerLen;
    std::vector<k4_cult_kmer> kmers(max_kmers);
    std::vector<uint8_t> bases((size_t)max_kmers * (size_t)(klen > 0 && klen <= cTotCultivarKMerLen ? klen : 1));
    std::vector<k4_cult_dist> dist(max_dist);
    const k4_cults_out out = {kmers.data(), bases.data(), dist.data()};
    const k4_cults_caps caps = {max_kmers, max_dist};
    std::vector<uint8_t> mem(sizeof(tsKMerCultsCnts), 0);
    tsKMerCultsCnts* pCnts = reinterpret_cast<tsKMerCultsCnts*>(mem.data());
    pCnts->TotCultivars = inf.n_entries;
    for (uint32_t i = 0; i < inf.n_entries && i < (uint32_t)cMaxCultivars; i++) pCnts->CultCnts[i].EntryID = i + 1;
    int64_t NumKMersLocated = 0;
    for (;;) {
      k4_cults_totals tot;
      {
        std::lock_guard<std::mutex> lk(m_Mtx);
        const int rc = k4_kmer_cults_batch(m_pIdx, &p, StartSfxIdx, EndSfxIdx, &out, &caps, &tot);
        if (rc != K4_OK) return Fail(rc);
      }
      NumKMersLocated += tot.n_located;
      for (uint64_t i = 0; i < tot.n_kmers; i++) {
        const k4_cult_kmer& k = kmers[i];
        pCnts->SenseCnts = k.sense_cnts; pCnts->AntisenseCnts = k.antisense_cnts; pCnts->NumCultivars = k.num_cultivars;
        memcpy(pCnts->KMerSeq, &bases[(size_t)i * klen], (size_t)klen);
        pCnts->KMerSeq[klen] = eBaseEOS;
        for (uint32_t j = 0; j < k.num_cultivars; j++) {
          const k4_cult_dist& d = dist[k.dist_ofs + j];
          pCnts->CultCnts[d.entry_id - 1].SenseCnts = d.sense;
          pCnts->CultCnts[d.entry_id - 1].AntisenseCnts = d.antisense;
        }
        const int Rslt = (*pCallback)(pThis, pCnts);
        if (Rslt < 0) return Rslt;
        for (uint32_t j = 0; j < k.num_cultivars; j++) {
          const k4_cult_dist& d = dist[k.dist_ofs + j];
          pCnts->CultCnts[d.entry_id - 1].SenseCnts = pCnts->CultCnts[d.entry_id - 1].AntisenseCnts = 0;
        }
      }
      if (tot.done) break;
      StartSfxIdx = (int64_t)tot.next_sfx_idx;
    }
    return NumKMersLocated;
  }

  // CSfxArray::LocateSfxHammings / LocateHammings, SfxArray.cpp:4107-4331 -- identical parameter lists (`ngskit4b hammings -m0`,
  // hammings.cpp:1692-1694).  One call is one device batch of one span; pHammings[0, nth, 2 nth ..] is written and nothing else.
  // The ident nodes are not needed.  0, or eBSFerrInternal (-1) where the reference returns it; K4_ERR_PARAMS for what the
  // device form does not take (RHamm above 10, a core KMerLen / (RHamm + 1) under 8 bases).  LocateHammings takes SeqEntry 0 only.
  int LocateSfxHammings(int RHamm, bool bSAHammings, int KMerLen, int SampleNth, int SrcSeqLen, uint32_t MinCoreDepth, uint32_t MaxCoreDepth,
                        uint32_t EntryID, uint32_t EntryLoci, int IntraInterBoth, uint8_t* pHammings, int NumAllocdIdentNodes = 0,
                        tsIdentNode* pAllocsIdentNodes = nullptr) {
    (void)NumAllocdIdentNodes; (void)pAllocsIdentNodes;
    if (!m_pIdx || EntryID == 0 || RHamm < 1 || KMerLen < 10 || KMerLen > 500 || SrcSeqLen < KMerLen || !pHammings) return K4_ERR_INTERNAL;
    const k4_hamming_params p = {RHamm, KMerLen, SampleNth, bSAHammings ? 1 : 0, MinCoreDepth, MaxCoreDepth, IntraInterBoth};
    const uint32_t len = (uint32_t)SrcSeqLen, nth = SampleNth > 0 ? (uint32_t)SampleNth : 1u;
    const uint64_t off = 0;
    std::lock_guard<std::mutex> dev(m_Mtx);
    const int rc = k4_locate_sfx_hammings_batch(m_pIdx, &p, 1, &EntryID, &EntryLoci, &len, &off, pHammings,
                                                (uint64_t)((len - (uint32_t)KMerLen) / nth) * nth + 1);
    return rc == K4_OK ? 0 : Fail(rc);
  }
  int LocateHammings(int RHamm, bool bSAHammings, int KMerLen, int SampleNth, int SrcSeqLen, uint32_t MinCoreDepth, uint32_t MaxCoreDepth,
                     etSeqBase* pSrcSeq, uint32_t SeqEntry, uint32_t SeqLoci, int IntraInterBoth, uint8_t* pHammings,
                     int NumAllocdIdentNodes = 0, tsIdentNode* pAllocsIdentNodes = nullptr) {
    (void)NumAllocdIdentNodes; (void)pAllocsIdentNodes; (void)SeqLoci;
    if (!m_pIdx || RHamm < 1 || KMerLen < 10 || KMerLen > 500 || SrcSeqLen < KMerLen || !pSrcSeq || !pHammings) return K4_ERR_INTERNAL;
    if (SeqEntry != 0) return K4_ERR_UNSUPPORTED;  // (a sequence of the index goes through LocateSfxHammings)
    const k4_hamming_params p = {RHamm, KMerLen, SampleNth, bSAHammings ? 1 : 0, MinCoreDepth, MaxCoreDepth, IntraInterBoth};
    const uint32_t len = (uint32_t)SrcSeqLen, nth = SampleNth > 0 ? (uint32_t)SampleNth : 1u;
    const uint64_t off = 0;
    std::lock_guard<std::mutex> dev(m_Mtx);
    const int rc = k4_locate_hammings_batch(m_pIdx, &p, 1, pSrcSeq, &off, &len, &off, pHammings,
                                            (uint64_t)((len - (uint32_t)KMerLen) / nth) * nth + 1);
    return rc == K4_OK ? 0 : Fail(rc);
  }

  // CSfxArray::IterateExacts, SfxArray.cpp:3381-3458 -- the five-argument form (`ngskit4b kmarkers`, LocKMers.cpp:1105).  PrevHitIdx 0
  // is one device batch of one probe (k4_exact_ranges_batch); otherwise the probe is compared on the host with the suffix at
  // PrevHitIdx, as CmpProbeTarg does (:2508-2525).  Returns the hit index (1..n), 0 without a (further) hit.
  int64_t IterateExacts(etSeqBase* pProbeSeq, uint32_t ProbeLen, int64_t PrevHitIdx, uint32_t* pTargEntryID, uint32_t* pHitLoci) {
    *pHitLoci = 0;
    *pTargEntryID = 0;
    k4_info_t inf;
    if (!m_pIdx || k4_info(m_pIdx, &inf) != K4_OK || PrevHitIdx < 0 || (uint64_t)PrevHitIdx >= inf.concat_len) return 0;
    uint64_t Idx = (uint64_t)PrevHitIdx, Psn = 0;
    std::lock_guard<std::mutex> dev(m_Mtx);
    if (!PrevHitIdx) {
      const uint64_t off = 0;
      uint32_t cnt = 0;
      if (k4_exact_ranges_batch(m_pIdx, 1, pProbeSeq, &off, &ProbeLen, &Idx, &cnt) != K4_OK) return Fail(0);
      if (!cnt) return 0;
    }
    if (k4_get_sfx_els(m_pIdx, Idx, 1, &Psn) != K4_OK) return Fail(0);
    if (PrevHitIdx) {
      std::vector<etSeqBase> Targ;
      ConcatBases(Psn, (int)ProbeLen, eBaseEOS, Targ);
      for (uint32_t k = 0; k < ProbeLen; k++)
        if ((Targ[k] & 0x0f) == eBaseEOS || (pProbeSeq[k] & 0x0f) != (Targ[k] & 0x0f)) return 0;
    }
    for (uint32_t e = 1; e <= inf.n_entries; e++) {
      k4_entry ent;
      if (k4_get_entry(m_pIdx, e, &ent) == K4_OK && ent.start_ofs <= Psn && Psn < ent.start_ofs + ent.seq_len) {
        *pTargEntryID = ent.entry_id;
        *pHitLoci = (uint32_t)(Psn - ent.start_ofs);
        return (int64_t)Idx + 1;
      }
    }
    return 0;
  }

  // CSfxArray::MatchesOtherChroms, SfxArray.cpp:5094-5235 -- both overloads, each one device batch of one probe: 1 when a core of
  // the probe hits an entry that is not among the ids where the probe can be laid over it, else 0; below 0 on errors.
  int MatchesOtherChroms(int NumProbeIDs, int* pProbeChromIDs, int MaxTotMM, int ProbeLen, etSeqBase* pProbe) {
    if (!m_pIdx || NumProbeIDs < 0 || ProbeLen < 0 || !pProbe) return K4_ERR_PARAMS;
    std::vector<uint32_t> Ids(pProbeChromIDs, pProbeChromIDs + NumProbeIDs);
    const uint64_t off = 0;
    const uint32_t len = (uint32_t)ProbeLen;
    int32_t m = 0;
    std::lock_guard<std::mutex> dev(m_Mtx);
    const int rc = k4_matches_other_chroms_batch(m_pIdx, NumProbeIDs, Ids.data(), MaxTotMM, 1, pProbe, &off, &len, &m);
    return rc == K4_OK ? m : Fail(rc);
  }
  int MatchesOtherChroms(int ProbeChromID, int MaxTotMM, int ProbeLen, etSeqBase* pProbe) {
    return MatchesOtherChroms(1, &ProbeChromID, MaxTotMM, ProbeLen, pProbe);
  }

  // The throughput form of `ngskit4b kmarkers` (CLocKMers::LocateSpeciesUniqueKMers as one thread runs it): one status byte per start
  // locus of every target, in the order of pTargetIDs, and the front end's tallies; k4sfx.h has the statuses.
  int SpeciesKMersBatch(const k4_kmarkers_params& Pars, int NumTargets, const uint32_t* pTargetIDs, uint8_t* pStatus, uint64_t StatusLen,
                        k4_kmarkers_totals* pTotals) {
    if (!m_pIdx) return K4_ERR_PARAMS;
    std::lock_guard<std::mutex> dev(m_Mtx);
    const int rc = k4_species_kmers_batch(m_pIdx, &Pars, NumTargets, pTargetIDs, pStatus, StatusLen, pTotals);
    return rc == K4_OK ? 0 : Fail(rc);
  }

  // CSfxArray::LocateAllNearMatches, SfxArray.h:823-837 -- identical parameter list (`genzygosity`, genzygosity.cpp:1193): one device
  // batch of one probe.  -1 when the probe is not unique to ProbeEntry or has more than MaxMatches matches elsewhere, else the
  // matches in other entries; a K4_ERR_* below -1 on errors.  pEntryMatches is zeroed and its first min(NumEntries, entries of the
  // index) places filled.  The ident-node scratch is not used; its count is honoured as the limit.  The probe is left as given.
  int LocateAllNearMatches(int MaxTotMM, int CoreLen, int CoreDelta, int MaxNumCoreSlides, int MaxMatches, int NumEntries, uint32_t* pEntryMatches,
                           uint32_t ProbeEntry, uint32_t ProbeOfs, int ProbeLen, etSeqBase* pProbeSeq, int CurMaxIter, int NumAllocdIdentNodes,
                           tsIdentNode* pAllocsIdentNodes) {
    (void)pAllocsIdentNodes;
    k4_info_t inf;
    if (!m_pIdx || k4_info(m_pIdx, &inf) != K4_OK || ProbeLen < 0 || !pProbeSeq) return K4_ERR_PARAMS;
    if (pEntryMatches && NumEntries >= 1) std::memset(pEntryMatches, 0, sizeof(uint32_t) * (size_t)NumEntries);
    const k4_near_params p = {MaxTotMM, CoreLen, CoreDelta, MaxNumCoreSlides, MaxMatches, CurMaxIter, NumAllocdIdentNodes, 0};
    const uint64_t off = 0;
    const uint32_t len = (uint32_t)ProbeLen;
    int32_t rslt = 0;
    std::vector<uint32_t> Counts(pEntryMatches && NumEntries >= 1 ? inf.n_entries : 0);
    std::lock_guard<std::mutex> dev(m_Mtx);
    const int rc = k4_all_near_matches_batch(m_pIdx, &p, 1, pProbeSeq, &off, &len, &ProbeEntry, &ProbeOfs, &rslt, Counts.empty() ? nullptr : Counts.data(),
                                             Counts.size());
    if (rc != K4_OK) return Fail(rc);
    for (size_t e = 0; e < Counts.size() && e < (size_t)NumEntries; e++) pEntryMatches[e] = Counts[e];
    return rslt;
  }

  // The throughput form of `genzygosity` (ThreadedCoredApprox over every window of the source entries): the sources x entries
  // matrix, the unique windows per source, optionally one status byte per start locus; k4sfx.h has the statuses.
  int ZygosityBatch(const k4_zygosity_params& Pars, int SrcFirst, int SrcCount, uint32_t* pMatrix, uint32_t* pSubseqs, uint8_t* pStatus,
                    uint64_t StatusLen, k4_zygosity_totals* pTotals) {
    if (!m_pIdx) return K4_ERR_PARAMS;
    std::lock_guard<std::mutex> dev(m_Mtx);
    const int rc = k4_zygosity_batch(m_pIdx, &Pars, SrcFirst, SrcCount, pMatrix, pSubseqs, pStatus, StatusLen, pTotals);
    return rc == K4_OK ? 0 : Fail(rc);
  }

  // CSfxArray::AlignPairedRead, SfxArray.h:880-896 -- identical parameter list (CKAligner's mate rescue,
  // KAligner.cpp:3372-3386,3476-3490).  -1 errors, 0 no match, 1 placed with mismatches only.
  int AlignPairedRead(bool b3primeExtend, bool bAntisense, uint32_t ChromID, uint32_t StartLoci, uint32_t EndLoci, int MinInsertSize,
                      int MaxInsertSize, int MaxAllowedMM, int MinHamming, int ReadLen, int MinChimericLen, int CoreLen,
                      int CoreDelta, int MaxNumCoreSlides, etSeqBase* pRead, tsHitLoci* pAlign) {
    (void)MinHamming; (void)MaxNumCoreSlides;
    if (!m_pIdx) return -1;
    k4_rescue_task t;
    std::memset(&t, 0, sizeof(t));
    t.chrom_id = ChromID; t.start_loci = StartLoci; t.end_loci = EndLoci; t.read_len = (uint32_t)ReadLen; t.read_off = 0;
    t.b3prime_extend = b3primeExtend ? 1 : 0; t.antisense = bAntisense ? 1 : 0;
    t.min_insert = MinInsertSize; t.max_insert = MaxInsertSize; t.max_allowed_mm = MaxAllowedMM;
    if (MinChimericLen >= 15 && MinChimericLen <= 99 && CoreLen > 0)  // chimeric mode: CoreLen / CoreDelta seed the wide windows
      t.chimeric = (uint32_t)MinChimericLen | ((uint32_t)(CoreLen > 4095 ? 4095 : CoreLen) << 8) |
                   ((uint32_t)(CoreDelta > 4095 ? 4095 : CoreDelta < 0 ? 0 : CoreDelta) << 20);
    int32_t rslt = 0;
    k4_hit h;
    std::lock_guard<std::mutex> lock(m_Mtx);
    int rc = k4_mate_rescue_batch(m_pIdx, 1, &t, pRead, (uint64_t)ReadLen, &rslt, &h);
    if (rc != K4_OK) return Fail(rc);
    if (rslt == 1 && pAlign) Expand(h, pAlign);
    return rslt;
  }

  // Batched form of the same call: n fresh reads, uniform parameters; pHits holds n * MaxHits records.
  int AlignReadsBatch(int TotMM, int CoreLen, int CoreDelta, int MaxNumCoreSlides, int MinCoreLen, int MMDelta,
                      eALStrand Align2Strand, int64_t NumReads, const etSeqBase* pReads, const uint64_t* pOffs,
                      const uint32_t* pLens, int MaxHits, int32_t* pRslts, int32_t* pLowHitInstances, int32_t* pLowMMCnt,
                      int32_t* pNxtLowMMCnt, k4_hit* pHits) {
    if (!m_pIdx) return K4_ERR_INTERNAL;
    k4_align_params p = {TotMM, CoreLen, CoreDelta, MaxNumCoreSlides, MinCoreLen, MMDelta, (int32_t)Align2Strand, MaxHits};
    int rc = k4_align_reads_batch(m_pIdx, &p, NumReads, pReads, pOffs, pLens, pRslts, pLowHitInstances, pLowMMCnt,
                                  pNxtLowMMCnt, pHits);
    return rc == K4_OK ? 0 : Fail(rc);
  }

  // CKAligner::AlignRead for a batch (ngskit4b/KAligner.cpp:9583-10105): per-read parameters + NAR classification.
  int KAlignBatch(const k4_kalign_params& Pars, int64_t NumReads, const etSeqBase* pReads, const uint64_t* pOffs,
                  const uint32_t* pLens, k4_read_result* pResults, k4_hit* pHits) {
    if (!m_pIdx) return K4_ERR_INTERNAL;
    int rc = k4_kalign_batch(m_pIdx, &Pars, NumReads, pReads, pOffs, pLens, pResults, pHits);
    return rc == K4_OK ? 0 : Fail(rc);
  }
};
#endif
