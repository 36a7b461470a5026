// kit4b_amd/csrc/k4_query.hip -- CSfxArray::LocateQuerySeqs (libkit4b/SfxArray.cpp:6493-6833, CBlitz's engine call) on gfx950:
// one WAVE per query sequence.  The reference walks the cores of a query in order, every occurrence of a core in suffix-array
// order, '+' before '-', and what it keeps of an occurrence depends on the nodes kept before it; the expensive parts -- counting a
// core's occurrences, mapping a suffix to its target, extending a seed -- do not.  So per group of 64 cores the lanes resolve one
// core each (k-mer table bucket, then the run's bounds inside it, no further than max_iter), the (core, occurrence) candidates of
// the group are laid out in the reference's order and taken 64 at a time: every lane maps its candidate, tests it against the
// nodes accepted before the chunk and extends it when it is not held by one; lane 0 then replays the chunk in order (containment
// against the nodes accepted inside the chunk, the redundancy rules, the append).  DESIGN.md "LocateQuerySeqs" has the rest.
#include <algorithm>
#include "k4_stage.h"

#define K4Q_CHAINS 256  // TargHash: (TargSeqID & 0x7f) << 1 | strand
#define K4Q_MAX_WS_BYTES (16ull << 30)

struct K4QNode {  // a node of a query's slice; its id (1-based, the reference's index into pHits + 1) is its place in the slice + 1
  uint32_t query_start, align_len, targ_seq_id, targ_loci, n_mismatches;
  uint32_t flags;  // bit 0 FlgStrand, bit 1 FlgRedundant
  uint32_t nxt;    // NxtHashMatch: id of the next older node of the same chain, 0 = none
  uint32_t pad;
};

struct K4QueryArgs {
  K4DevIndex ix;
  const uint8_t* seqs;
  const uint64_t* offs;
  const uint32_t* lens;
  int64_t n;
  k4_query_params p;
  K4QNode* ws;
  uint64_t slice;      // node slots per query
  uint32_t max_len;    // the query length the slices were sized for: a longer query yields nothing
  uint32_t* cnt;      // [2 n]: NumMatches, then the nodes left after the compaction (the host puts a zero behind them for its scan)
};

// :6605-6623: is the core (query offset ofs, locus loci of target tid) inside a node of the chain that starts at node id idx, on
// that node's diagonal?  Only the ids above `floor` are looked at (ids fall along a chain).
K4_DEV bool k4q_contained(const K4QNode* ws, uint32_t idx, uint32_t floor, uint32_t tid, uint32_t ofs, uint32_t loci, uint32_t cl) {
  while (idx > floor) {
    const K4QNode nd = ws[idx - 1];
    if (nd.targ_seq_id == tid && !(ofs < nd.query_start || ofs + cl > nd.query_start + nd.align_len) &&
        !(loci < nd.targ_loci || loci + cl > nd.targ_loci + nd.align_len) && ofs - nd.query_start == loci - nd.targ_loci)
      return true;
    idx = nd.nxt;
  }
  return false;
}

// :6628-6713: the 5' and the 3' extension of the core at query offset ofs / concatenation offset pos (locus loci of a target of
// seq_len bases)
K4_DEV void k4q_extend(K4Tb& tb, const K4QSeq& qs, const k4_query_params& p, uint32_t ofs, uint64_t pos, uint32_t loci, uint32_t seq_len,
                       uint32_t& flank5, uint32_t& flank3, int& mm5, int& mm3) {
  const int cl = p.core_len, mp = p.match_pts, xp = p.mismatch_pts;
  int n_mm = 0, score = cl * mp, floor_ = score - 4 * mp, hi_score = score, hi_mm = 0;
  uint32_t fl = 0, hi_len = 0;
  for (uint32_t k = min(loci, ofs); k > 0; k--) {
    const uint32_t tb_ = tb.get((int64_t)(pos - 1 - fl)) & 7u, pb = qs.at(ofs - 1 - fl) & 7u;
    if (tb_ > 4 || pb > 4) break;
    if (tb_ == 4 || pb == 4 || pb != tb_) {
      if (score >= floor_) {
        if (score > floor_) score -= xp;
        if (score < floor_) score = floor_;
      }
      n_mm++;
    } else
      score += mp;
    fl++;
    if (score >= hi_score && ((uint32_t)(n_mm * 100) / (fl + (uint32_t)cl)) <= 15) {
      hi_score = score; hi_len = fl; hi_mm = n_mm;
      floor_ = hi_score - 4 * mp;
    }
  }
  flank5 = hi_len; mm5 = hi_mm;
  n_mm = 0; score = cl * mp; floor_ = score - 4 * mp; hi_score = score; hi_mm = 0; fl = 0; hi_len = 0;
  for (uint32_t qi = ofs + (uint32_t)cl, ti = loci + (uint32_t)cl; qi < qs.len && ti < seq_len; qi++, ti++) {
    const uint32_t tb_ = tb.get((int64_t)(pos + (uint64_t)cl + fl)) & 7u, pb = qs.at(qi) & 7u;
    if (tb_ > 4 || pb > 4) break;
    if (tb_ == 4 || pb == 4 || pb != tb_) {
      if (score > floor_) score -= xp;
      if (score < floor_) score = floor_;
      n_mm++;
    } else
      score += mp;
    fl++;
    if (score >= hi_score && ((uint32_t)(n_mm * 100) / (fl + (uint32_t)cl)) <= 15) {
      hi_score = score; hi_len = fl; hi_mm = n_mm;
      floor_ = hi_score - 4 * mp;
    }
  }
  flank3 = hi_len; mm3 = hi_mm;
}

template <int EL>
__global__ void __launch_bounds__(64) k4k_query_locate(K4QueryArgs a) {
  __shared__ uint64_t ent_s[2 * K4_LDS_ENTRIES];
  __shared__ uint32_t entid_s[K4_LDS_ENTRIES];
  __shared__ uint32_t heads[K4Q_CHAINS];
  __shared__ uint64_t g_first[64];
  __shared__ uint32_t g_pre[65];
  __shared__ uint32_t c_ofs[64], c_tid[64], c_loci[64], c_qstart[64], c_alen[64], c_tloci[64], c_mm[64];
  __shared__ uint8_t c_ok[64];
  __shared__ uint32_t s_nm, s_stop;
  const int lane = threadIdx.x;
  const int64_t qi = blockIdx.x;
  const bool ent_in_lds = a.ix.n_entries <= K4_LDS_ENTRIES;
  if (ent_in_lds)
    for (int q = lane; q < (int)a.ix.n_entries; q += 64) {
      ent_s[q] = a.ix.ent_start[q];
      ent_s[K4_LDS_ENTRIES + q] = a.ix.ent_end[q];
      entid_s[q] = a.ix.ent_id[q];
    }
  for (int q = lane; q < K4Q_CHAINS; q += 64) heads[q] = 0;
  if (lane == 0) { s_nm = 0; s_stop = 0; }
  __syncthreads();
  const k4_query_params p = a.p;
  const uint32_t len = a.lens[qi], cl = (uint32_t)p.core_len, delta = (uint32_t)p.core_delta;
  const uint32_t max_iter = p.max_iter > 0 ? (uint32_t)p.max_iter : 0u, max_hits = (uint32_t)p.max_hits;
  K4QNode* ws = a.ws + (uint64_t)qi * a.slice;
  K4QSeq qs;
  qs.q = a.seqs + a.offs[qi];
  qs.len = len;
  K4Tb tb;
  tb.init(a.ix);
  // core offsets 0, delta, 2 delta .. below len - cl: the shrinking last step of the reference lands on len - cl, which its loop
  // test rejects (:6565-6571); a query no longer than the core has none
  const uint32_t span = len > cl && len <= a.max_len ? len - cl : 0u;
  const uint32_t n_cores = max_iter ? (uint32_t)(((uint64_t)span + delta - 1) / delta) : 0u;
  for (int s = (p.strand == 2 ? 1 : 0); s < (p.strand == 1 || p.strand == 3 ? 1 : 2) && !s_stop; s++) {
    qs.s = s;
    for (uint32_t gb = 0; gb < n_cores && !s_stop; gb += 64) {
      // 1. one core per lane: first index and count of its run
      const uint32_t ci = gb + (uint32_t)lane;
      uint64_t first = 0;
      uint32_t cnt = 0;
      if (ci < n_cores) {
        cnt = k4q_count<EL>(a.ix, tb, qs, ci * delta, (int)cl, max_iter, first);
        if (cnt >= max_iter) cnt = 0;  // :6590
      }
      k4d_runs_layout(lane, first, cnt, g_first, g_pre);
      __syncthreads();
      const uint32_t total = g_pre[64];
      // 2. the candidates in the reference's order, 64 at a time
      for (uint32_t c0 = 0; c0 < total && !s_stop; c0 += 64) {
        const uint32_t g = c0 + (uint32_t)lane;
        const uint32_t nm0 = s_nm;
        bool ok = false;
        if (g < total) {
          uint32_t core, occ;
          k4d_runs_locate(g, 63u, g_pre, core, occ);  // (the lanes behind the group's last core hold no candidate)
          const uint32_t ofs = (gb + core) * delta;
          const uint64_t pos = k4d_sa_at<EL>(a.ix, g_first[core] + occ);
          uint64_t e_start, e_end;
          const int e = k4d_map_entry_slow(a.ix, ent_in_lds ? ent_s : nullptr, pos, e_start, e_end);
          if (e >= 0) {
            const uint32_t tid = ent_in_lds ? entid_s[e] : a.ix.ent_id[e];
            const uint32_t loci = (uint32_t)(pos - e_start);
            c_ofs[lane] = ofs; c_tid[lane] = tid; c_loci[lane] = loci;
            ok = !k4q_contained(ws, heads[((tid & 0x7fu) << 1) | (uint32_t)s], 0u, tid, ofs, loci, cl);
            if (ok) {
              uint32_t f5, f3;
              int m5, m3;
              k4q_extend(tb, qs, p, ofs, pos, loci, (uint32_t)(e_end - e_start + 1), f5, f3, m5, m3);
              c_qstart[lane] = ofs - f5; c_tloci[lane] = loci - f5; c_alen[lane] = f5 + cl + f3; c_mm[lane] = (uint32_t)(m5 + m3);
            }
          }
        }
        c_ok[lane] = ok ? 1 : 0;
        __syncthreads();
        // 3. the chunk in order
        if (lane == 0) {
          uint32_t nm = nm0;
          const uint32_t nc = min(64u, total - c0);
          for (uint32_t l = 0; l < nc; l++) {
            if (!c_ok[l]) continue;
            const uint32_t tid = c_tid[l], h = ((tid & 0x7fu) << 1) | (uint32_t)s;
            if (k4q_contained(ws, heads[h], nm0, tid, c_ofs[l], c_loci[l], cl)) continue;
            K4QNode cur;
            cur.query_start = c_qstart[l]; cur.align_len = c_alen[l]; cur.targ_seq_id = tid; cur.targ_loci = c_tloci[l];
            cur.n_mismatches = c_mm[l]; cur.flags = (uint32_t)s; cur.nxt = heads[h]; cur.pad = 0;
            bool red = false;
            for (uint32_t idx = heads[h]; idx != 0;) {  // :6734-6775
              const K4QNode pv = ws[idx - 1];
              bool pv_red = false;
              if (!(pv.flags & 2u) && (pv.flags & 1u) == (uint32_t)s && pv.targ_seq_id == tid &&
                  !((cur.query_start + cur.align_len + cl - 1) < pv.query_start || cur.query_start > (pv.query_start + pv.align_len + cl - 1))) {
                if ((cur.align_len + cl / 2) <= pv.align_len) red = true;
                else if (cur.align_len >= (pv.align_len + cl / 2)) pv_red = true;
                if (!((cur.targ_loci + cur.align_len + cl - 1) < pv.targ_loci || cur.targ_loci > (pv.targ_loci + pv.align_len + cl - 1))) {
                  if (cur.align_len < pv.align_len) red = true;
                  else if (cur.align_len > pv.align_len) pv_red = true;
                  else if (cur.n_mismatches >= pv.n_mismatches) red = true;
                  else pv_red = true;
                }
              }
              if (pv_red) ws[idx - 1].flags = pv.flags | 2u;
              idx = pv.nxt;
            }
            if (red) continue;
            ws[nm] = cur;  // (nm < max_hits <= slice)
            nm++;
            heads[h] = nm;
            if (nm >= max_hits) { s_stop = 1; break; }
          }
          s_nm = nm;
        }
        __syncthreads();
      }
      __syncthreads();  // (g_first / g_pre are rewritten by the next group)
    }
  }
  __syncthreads();
  const uint32_t nm = s_nm;
  uint32_t kept = 0;
  for (uint32_t j = (uint32_t)lane; j < nm; j += 64) kept += (ws[j].flags & 2u) ? 0u : 1u;
  kept = k4d_wave_sum(kept);
  if (lane == 0) { a.cnt[qi] = nm; a.cnt[a.n + qi] = kept; }
}

// :6803-6824: the nodes that are not flagged, in slice order, behind one another; nothing when they do not all fit
__global__ void __launch_bounds__(64) k4k_query_gather(const K4QNode* __restrict__ ws_all, uint64_t slice, const uint32_t* __restrict__ cnt,
                                                       int64_t n, const uint64_t* __restrict__ node_offs, k4_query_node* __restrict__ nodes,
                                                       uint64_t nodes_cap) {
  if (node_offs[n] > nodes_cap) return;
  const int64_t qi = blockIdx.x;
  const int lane = threadIdx.x;
  const K4QNode* ws = ws_all + (uint64_t)qi * slice;
  const uint32_t nm = cnt[qi];
  uint64_t out = node_offs[qi];
  for (uint32_t j0 = 0; j0 < nm; j0 += 64) {
    const uint32_t j = j0 + (uint32_t)lane;
    K4QNode nd;
    bool keep = false;
    if (j < nm) { nd = ws[j]; keep = !(nd.flags & 2u); }
    const unsigned long long m = __ballot(keep);
    if (keep) {
      k4_query_node o;
      o.query_start = nd.query_start; o.align_len = nd.align_len; o.targ_seq_id = nd.targ_seq_id; o.targ_loci = nd.targ_loci;
      o.n_mismatches = nd.n_mismatches; o.slot = j; o.strand = nd.flags & 1u;
      nodes[out + (uint64_t)__popcll(m & ((1ull << lane) - 1ull))] = o;
    }
    out += (uint64_t)__popcll(m);
  }
}

// ==== host side ======================================================================================================
static int check_query_params(k4_index* ix, const k4_query_params* p) {
  if (!ix || !p) return K4_ERR_PARAMS;
  if (p->core_len < 8 || p->core_len > 100) return k4_fail(ix, K4_ERR_PARAMS, "LocateQuerySeqs: core_len %d outside 8..100", p->core_len);
  if (p->core_delta < 1) return k4_fail(ix, K4_ERR_PARAMS, "LocateQuerySeqs: core_delta %d below 1", p->core_delta);
  if (p->max_hits < 1) return k4_fail(ix, K4_ERR_PARAMS, "LocateQuerySeqs: max_hits %d below 1", p->max_hits);
  if (p->strand < 0 || p->strand > 3) return k4_fail(ix, K4_ERR_PARAMS, "LocateQuerySeqs: strand %d outside 0..3", p->strand);
  return K4_OK;
}

// node slots a query of up to max_len bases can fill: never more than max_hits, nor than its candidates
static uint64_t query_slice(const k4_query_params* p, uint32_t max_len) {
  const uint64_t span = max_len > (uint32_t)p->core_len ? max_len - (uint32_t)p->core_len : 0;
  const uint64_t cores = (span + (uint64_t)p->core_delta - 1) / (uint64_t)p->core_delta;
  const uint64_t cands = 2 * cores * (uint64_t)(p->max_iter > 1 ? p->max_iter - 1 : 0);
  return std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)p->max_hits, cands));
}

extern "C" int k4_query_reserve(k4_index* ix, const k4_query_params* p, int64_t max_queries, uint32_t max_query_len) {
  int rc = check_query_params(ix, p);
  if (rc != K4_OK) return rc;
  if (max_queries < 0 || max_queries >= 0x7FFFFFFFll) return k4_fail(ix, K4_ERR_PARAMS, "LocateQuerySeqs: at most 2^31-2 queries per batch");
  K4_HIP(ix, hipSetDevice(ix->device));
  K4QueryState& q = ix->qry;
  const uint64_t slice = query_slice(p, max_query_len);
  if (max_queries <= q.cap_queries && slice <= q.cap_slice) return K4_OK;
  const int64_t nq = std::max<int64_t>(std::max<int64_t>(max_queries, q.cap_queries), 1);
  const uint64_t sl = std::max<uint64_t>(slice, q.cap_slice);
  if ((uint64_t)nq * sl > K4Q_MAX_WS_BYTES / sizeof(K4QNode))
    return k4_fail(ix, K4_ERR_MEM, "LocateQuerySeqs: %lld queries x %llu node slots exceed the %llu GiB workspace limit: split the batch or lower max_hits",
                   (long long)nq, (unsigned long long)sl, (unsigned long long)(K4Q_MAX_WS_BYTES >> 30));
  q.cap_queries = 0;  // (zero until both have grown, K4DevBuf::reserve)
  q.cap_slice = 0;
  K4_HIP(ix, hipDeviceSynchronize());  // (a block about to be replaced may still be read by a batch on a caller's stream)
  K4_HIP(ix, q.ws.reserve((size_t)nq * sl * sizeof(K4QNode)));
  K4_HIP(ix, q.cnt.reserve(((size_t)nq * 2 + 1) * sizeof(uint32_t)));
  q.cap_queries = nq;
  q.cap_slice = sl;
  return K4_OK;
}

extern "C" int k4_locate_query_seqs_batch_dev(k4_index* ix, const k4_query_params* p, int64_t n, uint32_t max_query_len, const void* d_seqs,
                                              const void* d_offs, const void* d_lens, void* d_node_offs, void* d_nodes, uint64_t nodes_cap,
                                              void* stream) {
  int rc = check_query_params(ix, p);
  if (rc != K4_OK) return rc;
  K4QueryState& q = ix->qry;
  q.timer.reset();
  if (n < 0 || !d_node_offs || (n > 0 && (!d_seqs || !d_offs || !d_lens))) return k4_fail(ix, K4_ERR_PARAMS, "LocateQuerySeqs: null argument");
  if (nodes_cap > 0 && !d_nodes) return k4_fail(ix, K4_ERR_PARAMS, "LocateQuerySeqs: nodes_cap without nodes");
  if ((rc = k4_query_reserve(ix, p, n, max_query_len)) != K4_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  uint64_t* node_offs = (uint64_t*)d_node_offs;
  K4QueryArgs a;
  a.ix = ix->d;
  a.seqs = (const uint8_t*)d_seqs; a.offs = (const uint64_t*)d_offs; a.lens = (const uint32_t*)d_lens;
  a.n = n; a.p = *p;
  a.ws = q.ws.as<K4QNode>();
  a.slice = query_slice(p, max_query_len);
  a.max_len = max_query_len;
  a.cnt = q.cnt.as<uint32_t>();
  if (n > 0) {  // (a batch of no queries has no work to time)
    K4_HIP(ix, q.timer.begin(st));
    K4S_LAUNCH_EL(ix, k4k_query_locate, (unsigned)n, 64, st, a);
  }
  // node_offs[0 .. n] from the counts of the nodes kept, cnt[n .. 2 n), and a zero behind them
  K4_HIP(ix, hipMemsetAsync(a.cnt + 2 * n, 0, 4, st));
  K4_TRY(k4s_exclusive_scan<K4DevBuf>(ix, a.cnt + n, node_offs, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st, &q.scan));
  if (n > 0)
    hipLaunchKernelGGL(k4k_query_gather, dim3((unsigned)n), dim3(64), 0, st, a.ws, a.slice, a.cnt, n, node_offs, (k4_query_node*)d_nodes, nodes_cap);
  K4_HIP(ix, hipGetLastError());
  K4_HIP(ix, q.timer.end(st));
  uint64_t total = 0;
  K4_TRY(k4s_read_back(ix, &total, node_offs + n, st));
  K4_HIP(ix, q.timer.read());
  if (total > nodes_cap)
    return k4_fail(ix, K4_ERR_MEM, "LocateQuerySeqs: %llu nodes found, nodes_cap is %llu", (unsigned long long)total, (unsigned long long)nodes_cap);
  return K4_OK;
}

extern "C" int k4_locate_query_seqs_batch(k4_index* ix, const k4_query_params* p, int64_t n, const uint8_t* seqs, const uint64_t* offs,
                                          const uint32_t* lens, uint64_t* node_offs, k4_query_node* nodes, uint64_t nodes_cap) {
  int rc = check_query_params(ix, p);
  if (rc != K4_OK) return rc;
  ix->qry.timer.reset();
  if (n < 0 || !node_offs || (n > 0 && (!seqs || !offs || !lens)) || (nodes_cap > 0 && !nodes))
    return k4_fail(ix, K4_ERR_PARAMS, "LocateQuerySeqs: null argument");
  K4SeqStage& s = ix->seq_stage;
  hipStream_t st;
  K4_TRY(k4s_call_open(ix, &st));
  uint32_t max_len = 0;
  K4_TRY(k4s_stage_seqs(ix, n, seqs, offs, lens, &max_len));
  if ((rc = k4_query_reserve(ix, p, n, max_len)) != K4_OK) return rc;  // (so that K4_ERR_MEM below can only mean nodes_cap)
  K4_HIP(ix, s.node_offs.reserve((size_t)(n + 1) * 8));
  K4_HIP(ix, s.nodes.reserve((size_t)std::max<uint64_t>(nodes_cap, 1) * sizeof(k4_query_node)));
  rc = k4_locate_query_seqs_batch_dev(ix, p, n, max_len, s.seqs.p, s.offs.p, s.lens.p, s.node_offs.p, s.nodes.p, nodes_cap, st);
  if (rc != K4_OK && rc != K4_ERR_MEM) return rc;
  K4_HIP(ix, hipMemcpyAsync(node_offs, s.node_offs.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
  K4_TRY(k4s_call_close(ix, st, ix->qry.timer));
  if (rc != K4_OK) return rc;
  if (node_offs[n]) K4_HIP(ix, hipMemcpy(nodes, s.nodes.p, (size_t)node_offs[n] * sizeof(k4_query_node), hipMemcpyDeviceToHost));
  return K4_OK;
}

extern "C" double k4_query_last_kernel_ms(const k4_index* ix) { return ix ? ix->qry.timer.ms : 0.0; }
