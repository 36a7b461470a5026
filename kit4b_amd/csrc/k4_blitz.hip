// kit4b_amd/csrc/k4_blitz.hip -- CBlitz's path stage (libkit4b/CBlitz.cpp) on gfx950: what `ngskit4b blitz` does between the nodes
// CSfxArray::LocateQuerySeqs returned for a query (k4_query.hip) and its PSL line.
//   opener   the batch's nodes sorted by query, target, strand, query start, locus (SortQueryAlignNodes :3596): two stable
//            k4s_sort_pairs passes, the low half of the key first
//   score    one WAVE per (query, target group, strand): the inner IdentifyHighScorePaths (:1641-1725) with HighScoreSW (:1560-1635)
//            filled from the back of the sorted group instead of by recursion; a group is what the outer routine (:2603-2663)
//            hands to one call, the last node of a query that stands alone on a new target included
//   pick     one wave per query: its heads by score descending, target ascending, the first max_paths of them
//   path     one wave per reported path: ConsolidateNodes (:2157-2320) and CharacterisePath (:2666-2779) by lane 0, the counts of
//            BlocksAlignStats (:1729-1849) across the lanes
// DESIGN.md "blitz: the path stage" has the rest.
#include <algorithm>
#include "k4_stage.h"

struct K4BNode {  // a node of the sorted batch; nxt: place in the sorted batch + 1 of the next node of its path, 0 = none
  uint32_t qs, al, tid, tl, mm, flags, score, nxt;
};
enum : uint32_t { K4B_STRAND = 1u, K4B_RPT = 2u, K4B_FIRST = 4u, K4B_GROUP = 8u, K4B_TAKEN = 16u };
#define K4B_OVERLAP_FLOAT 8u   // cMaxBlitzOverlapFloat
#define K4B_MAX_GAP 500000u    // cGapBlitzMaxLength

// ---- opener ---------------------------------------------------------------------------------------------------------
// the low half of the key (query start, locus), the node's place as the value, and the query each node belongs to
__global__ void __launch_bounds__(256) k4k_blitz_keys_lo(const k4_query_node* __restrict__ nodes, const uint64_t* __restrict__ node_offs, int64_t n,
                                                         uint64_t total, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                         uint32_t* __restrict__ qi) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  int64_t lo = 0, hi = n - 1;  // the last query whose nodes start at or before i
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (node_offs[mid] <= i) lo = mid; else hi = mid - 1;
  }
  keys[i] = ((uint64_t)nodes[i].query_start << 32) | nodes[i].targ_loci;
  vals[i] = (uint32_t)i;
  qi[i] = (uint32_t)lo;
}

// the high half: query, target, strand
__global__ void __launch_bounds__(256) k4k_blitz_keys_hi(const k4_query_node* __restrict__ nodes, const uint32_t* __restrict__ qi,
                                                         const uint32_t* __restrict__ vals, uint64_t total, uint64_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const uint32_t v = vals[i];
  keys[i] = ((uint64_t)qi[v] << 33) | ((uint64_t)nodes[v].targ_seq_id << 1) | (nodes[v].strand & 1u);
}

// the nodes in sorted order; K4B_GROUP on the first node of what the outer IdentifyHighScorePaths hands to one call: a query's
// first node, and every node whose target differs from the one before it unless it is the query's last node (:2632-2648)
__global__ void __launch_bounds__(256) k4k_blitz_gather(const k4_query_node* __restrict__ nodes, const uint32_t* __restrict__ qi,
                                                        const uint32_t* __restrict__ vals, const uint64_t* __restrict__ node_offs,
                                                        uint64_t total, K4BNode* __restrict__ ws) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const uint32_t v = vals[i];
  const k4_query_node nd = nodes[v];
  const uint32_t q = qi[v];
  K4BNode o;
  o.qs = nd.query_start; o.al = nd.align_len; o.tid = nd.targ_seq_id; o.tl = nd.targ_loci; o.mm = nd.n_mismatches;
  o.flags = nd.strand & 1u; o.score = 0; o.nxt = 0;
  if (i == node_offs[q] || (nodes[vals[i - 1]].targ_seq_id != nd.targ_seq_id && i + 1 != node_offs[q + 1])) o.flags |= K4B_GROUP;
  ws[i] = o;
}

struct K4BHasFlag {
  const K4BNode* ws;
  uint32_t flag;
  __device__ bool operator()(uint32_t i) const { return (ws[i].flags & flag) != 0; }
};

// ---- score ----------------------------------------------------------------------------------------------------------
struct K4BlitzArgs {
  K4DevIndex ix;
  const uint8_t* seqs;
  const uint64_t* offs;
  const uint32_t* lens;
  const uint64_t* node_offs;
  int64_t n;
  k4_blitz_params p;
  K4BNode* ws;
  const uint32_t* qi;      // query of the node at place vals[i] of the caller's array
  const uint32_t* vals;    // sorted place -> caller's place
  uint64_t total;
};

// (int)sqrt((double)q * q + (double)t * t) of :1611 as an exact integer floor square root: both squares stay below 2^50
K4_DEV uint32_t k4b_gap_len(uint32_t q, uint32_t t) {
  const uint64_t s = (uint64_t)q * q + (uint64_t)t * t;
  uint64_t r = (uint64_t)sqrt((double)s);
  while (r * r > s) r--;
  while ((r + 1) * (r + 1) <= s) r++;
  return (uint32_t)r;
}

K4_DEV uint32_t k4b_own_score(const K4BNode& nd, const k4_blitz_params& p) {
  const uint32_t s = nd.al * (uint32_t)p.match_pts, m = nd.mm * (uint32_t)p.mismatch_pts;
  return m >= s ? 0u : s - m;
}

__global__ void __launch_bounds__(64) k4k_blitz_score(K4BlitzArgs a, const uint32_t* __restrict__ groups, uint64_t n_groups) {
  __shared__ uint32_t s_best, s_n_put;
  const int lane = threadIdx.x;
  const uint32_t s = blockIdx.y;  // 0 sense, 1 antisense
  if ((s == 0 && a.p.strand == 2) || (s == 1 && a.p.strand == 1)) return;
  const uint64_t g = blockIdx.x;
  const uint64_t lo = groups[g], hi = g + 1 < n_groups ? groups[g + 1] : a.total;
  K4BNode* ws = a.ws;
  const k4_blitz_params p = a.p;
  const uint32_t qlen = a.lens[a.qi[a.vals[lo]]];
  // A node is at least core_len >= 8 bases, so LocateQuerySeqs has none for a query under 8; caller-made nodes on one are ignored
  // (the whole wave leaves).  This keeps the automatic minimum (:1539-1542) positive and the percentage's divisor non-zero.
  if (qlen < 8u) return;
  uint32_t mps = p.min_path_score > 0 ? (uint32_t)p.min_path_score : (uint32_t)(((uint64_t)(qlen - 5u) * (uint32_t)p.match_pts) / 3u);
  if (mps < 25u) mps = 25u;  // (:1658)
  if (lane == 0) s_n_put = 0;
  __syncthreads();
  for (;;) {
    // HighScoreSW for every node of the strand that is not on a path yet, from the back: a successor starts no earlier than its
    // predecessor on the query, and no earlier on the target where it starts at the same query offset, so it lies behind it
    for (uint64_t i = hi; i-- > lo;) {
      const K4BNode c = ws[i];
      if ((c.flags & K4B_RPT) || (c.flags & K4B_STRAND) != s) continue;
      const uint32_t own = k4b_own_score(c, p);
      const uint32_t t_lo = c.tl + c.al - K4B_OVERLAP_FLOAT, t_hi = c.tl + c.al + K4B_MAX_GAP, q_lo = c.qs + c.al - K4B_OVERLAP_FLOAT;
      uint32_t best = 0, best_j = 0xFFFFFFFFu;
      for (uint64_t j0 = i + 1; j0 < hi; j0 += 64) {
        const uint64_t j = j0 + (uint64_t)lane;
        if (j >= hi) continue;
        const K4BNode e = ws[j];
        if (e.tid != c.tid || (e.flags & K4B_RPT) || (e.flags & K4B_STRAND) != s) continue;
        if (e.tl < t_lo || e.tl > t_hi || e.qs < q_lo) continue;
        const int32_t qg = (int32_t)(e.qs - (c.qs + c.al)), tg = (int32_t)(e.tl - (c.tl + c.al));
        const uint32_t gl = k4b_gap_len((uint32_t)(qg < 0 ? -qg : qg), (uint32_t)(tg < 0 ? -tg : tg));
        uint32_t gap = 1u + gl / 10u;
        if (gap > 10u) gap = 10u;
        gap += (uint32_t)p.gap_open;
        uint32_t put = e.score + own;
        put = gap >= put ? 0u : put - gap;
        if (put > best) { best = put; best_j = (uint32_t)j; }
      }
      for (int d = 32; d > 0; d >>= 1) {  // the highest score, the lowest place among equals
        const uint32_t ob = __shfl_xor(best, d, 64), oj = __shfl_xor(best_j, d, 64);
        if (ob > best || (ob == best && oj < best_j)) { best = ob; best_j = oj; }
      }
      if (lane == 0) {
        ws[i].score = best > 0 ? best : own;
        ws[i].nxt = best > 0 ? best_j + 1u : 0u;
      }
      __syncthreads();  // (the nodes in front of i read this score)
    }
    // the best head: a strictly greater score wins, so the lowest place among equals
    uint32_t best = 0, best_i = 0xFFFFFFFFu;
    for (uint64_t i = lo + (uint64_t)lane; i < hi; i += 64) {
      const K4BNode c = ws[i];
      if ((c.flags & K4B_RPT) || (c.flags & K4B_STRAND) != s) continue;
      if (c.score > best) { best = c.score; best_i = (uint32_t)i; }
    }
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t ob = __shfl_xor(best, d, 64), oi = __shfl_xor(best_i, d, 64);
      if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
    }
    if (lane == 0) {
      uint32_t b = best;
      if (b >= mps) {
        uint32_t al = 0;
        for (uint32_t k = best_i + 1u; k != 0; k = ws[k - 1].nxt) al += ws[k - 1].al;
        if ((al * 100u) / qlen >= (uint32_t)p.query_len_aligned_pct) {
          for (uint32_t k = best_i + 1u; k != 0; k = ws[k - 1].nxt) ws[k - 1].flags |= K4B_RPT;
          ws[best_i].flags |= K4B_FIRST;
          s_n_put++;
        } else
          b = 0;  // (a best path under the cut ends the group's loop, :1718-1722)
      }
      s_best = b;
    }
    __syncthreads();
    if (!(s_best >= mps && s_n_put < (uint32_t)p.max_paths)) break;
  }
}

// ---- pick -----------------------------------------------------------------------------------------------------------
// per query: its heads (their places ascending in `heads`) by score descending, target ascending, place ascending; the first
// max_paths of them go to sel[q * max_paths ..], their number to cnt[q]
__global__ void __launch_bounds__(64) k4k_blitz_pick(K4BNode* __restrict__ ws, const uint32_t* __restrict__ heads, uint64_t n_heads,
                                                     const uint64_t* __restrict__ node_offs, int64_t n, int max_paths, uint32_t* __restrict__ sel,
                                                     uint32_t* __restrict__ cnt) {
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x;
  if (q == n) {  // (the scan behind this kernel runs over n + 1 counts)
    if (lane == 0) cnt[n] = 0;
    return;
  }
  uint64_t b[2];
  for (int k = 0; k < 2; k++) {  // the first head at or behind the query's first / the next query's first node
    const uint64_t key = node_offs[q + k];
    uint64_t lo = 0, hi = n_heads;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (heads[mid] < key) lo = mid + 1; else hi = mid;
    }
    b[k] = lo;
  }
  const uint32_t keep = b[1] - b[0] < (uint64_t)max_paths ? (uint32_t)(b[1] - b[0]) : (uint32_t)max_paths;
  for (uint32_t r = 0; r < keep; r++) {
    uint32_t sc = 0, tid = 0xFFFFFFFFu, at = 0xFFFFFFFFu;
    for (uint64_t h = b[0] + (uint64_t)lane; h < b[1]; h += 64) {
      const K4BNode c = ws[heads[h]];
      if (c.flags & K4B_TAKEN) continue;
      if (at == 0xFFFFFFFFu || c.score > sc || (c.score == sc && c.tid < tid)) { sc = c.score; tid = c.tid; at = heads[h]; }
    }
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t os = __shfl_xor(sc, d, 64), ot = __shfl_xor(tid, d, 64), oa = __shfl_xor(at, d, 64);
      if (oa != 0xFFFFFFFFu && (at == 0xFFFFFFFFu || os > sc || (os == sc && (ot < tid || (ot == tid && oa < at))))) { sc = os; tid = ot; at = oa; }
    }
    if (lane == 0) {
      ws[at].flags |= K4B_TAKEN;
      sel[(uint64_t)q * (uint64_t)max_paths + r] = at;
    }
    __syncthreads();
  }
  if (lane == 0) cnt[q] = keep;
}

// ---- path -----------------------------------------------------------------------------------------------------------
struct K4BSeqs {  // the path's target (bases of entry [start, start + len)) and the query in the path's orientation
  K4Tb tb;
  uint64_t start;
  uint32_t len;
  K4QSeq qs;
  K4_DEV uint32_t t(uint32_t loci) { return loci < len ? tb.get((int64_t)(start + loci)) & 0x0Fu : 0xFFu; }  // GetBase (SfxArray.cpp:2367)
  K4_DEV uint32_t q(uint32_t j) const { return j < qs.len ? qs.at(j) : 0xFEu; }
};

// ConsolidateNodes (:2157-2320) from the head at place `head`
K4_DEV void k4b_consolidate(K4BNode* ws, uint32_t head, K4BSeqs& sq) {
  K4BNode* cur = &ws[head];
  while (cur->nxt != 0) {
    K4BNode* nx = &ws[cur->nxt - 1];
    uint32_t c_al = cur->al, n_al = nx->al, n_qs = nx->qs, n_tl = nx->tl;
    const uint32_t c_qs = cur->qs, c_tl = cur->tl;
    const int64_t dq = (int64_t)n_qs - (int64_t)(uint64_t)(uint32_t)(c_qs + c_al - 1u), dt = (int64_t)n_tl - (int64_t)(uint64_t)(uint32_t)(c_tl + c_al - 1u);
    int64_t delta = (dq < 0 ? -dq : dq) <= (dt < 0 ? -dt : dt) ? dq : dt;
    if (delta > 1) {  // close the gap
      uint32_t cp = c_qs + c_al, np = n_qs - 1u, ct = c_tl + c_al, nt = n_tl - 1u;
      while (delta-- > 1) {
        const bool cm0 = sq.q(cp) == sq.t(ct), nm0 = sq.q(np) == sq.t(nt);
        const bool cm = cm0 == nm0 ? (delta & 1) != 0 : cm0;
        if (cm) { c_al++; ct++; cp++; }
        else { n_al++; n_qs--; n_tl--; nt--; np--; }
      }
    } else if (delta < 0) {  // trim the overlap
      uint32_t cp = c_qs + c_al - 1u, np = n_qs, ct = c_tl + c_al - 1u, nt = n_tl;
      while (delta++ < 1) {
        const bool cm0 = sq.q(cp) == sq.t(ct), nm0 = sq.q(np) == sq.t(nt);
        const bool nm = cm0 == nm0 ? (delta & 1) != 0 : nm0;
        if (nm) { c_al--; ct--; cp--; }
        else { n_al--; n_qs++; n_tl++; nt++; np++; }
      }
    }
    cur->al = c_al;
    nx->al = n_al; nx->qs = n_qs; nx->tl = n_tl;
    if (c_al == 0) { cur->nxt = nx->nxt; cur->al = n_al; continue; }
    if (n_al == 0) { cur->nxt = nx->nxt; continue; }
    if ((int64_t)n_qs - (int64_t)(uint64_t)(uint32_t)(c_qs + c_al - 1u) == 1 && (int64_t)n_tl - (int64_t)(uint64_t)(uint32_t)(c_tl + c_al - 1u) == 1) {
      cur->nxt = nx->nxt;
      cur->al = c_al + n_al;
      continue;
    }
    cur = nx;
  }
}

__global__ void __launch_bounds__(64) k4k_blitz_path(K4BlitzArgs a, const uint32_t* __restrict__ sel, const uint32_t* __restrict__ cnt,
                                                     const uint64_t* __restrict__ path_offs, k4_blitz_path* __restrict__ out,
                                                     uint32_t* __restrict__ n_blocks) {
  __shared__ uint32_t s_e;
  const int lane = threadIdx.x;
  const int64_t q = blockIdx.x;
  const uint32_t r = blockIdx.y;
  if (q == a.n) {  // (the scan behind this kernel runs over one count more than there are paths)
    if (lane == 0 && r == 0) n_blocks[path_offs[a.n]] = 0;
    return;
  }
  if (r >= cnt[q]) return;
  K4BNode* ws = a.ws;
  const uint32_t head = sel[(uint64_t)q * (uint64_t)a.p.max_paths + r];
  const K4BNode hd0 = ws[head];
  // The target's entry.  Entry ids come from the index file and need not be the entry's place + 1, though they usually are: that
  // place is tried first.  Otherwise the table is scanned; ids are unique, so at most one lane writes s_e.
  uint32_t e = hd0.tid - 1u;
  if (!(e < a.ix.n_entries && a.ix.ent_id[e] == hd0.tid)) {
    if (lane == 0) s_e = 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t k = (uint32_t)lane; k < a.ix.n_entries; k += 64)
      if (a.ix.ent_id[k] == hd0.tid) s_e = k;
    __syncthreads();
    e = s_e;
  }
  K4BSeqs sq;
  sq.tb.init(a.ix);
  sq.start = e != 0xFFFFFFFFu ? a.ix.ent_start[e] : 0;
  sq.len = e != 0xFFFFFFFFu ? (uint32_t)(a.ix.ent_end[e] - a.ix.ent_start[e] + 1) : 0u;
  sq.qs.q = a.seqs + a.offs[q];
  sq.qs.len = a.lens[q];
  sq.qs.s = (int)(hd0.flags & K4B_STRAND);
  k4_blitz_path o;
  uint32_t nb = 1;
  if (lane == 0) {
    k4b_consolidate(ws, head, sq);
    // CharacterisePath: the second overlap trim (:2719-2742), then the inserts and the ends (:2744-2764)
    const K4BNode h = ws[head];
    uint32_t qe = h.qs + h.al - 1u, te = h.tl + h.al - 1u;
    for (uint32_t k = h.nxt; k != 0; k = ws[k - 1].nxt) {
      K4BNode* t = &ws[k - 1];
      const int64_t qg = (int64_t)t->qs - (int64_t)qe - 1, tg = (int64_t)t->tl - (int64_t)te - 1;
      if (qg < 0 || tg < 0) {
        const uint32_t d = (uint32_t)(qg >= 0 ? -tg : tg >= 0 ? -qg : -(qg < tg ? qg : tg));
        t->qs += d; t->tl += d; t->al -= d;
      }
      qe = t->qs + t->al - 1u; te = t->tl + t->al - 1u;
    }
    qe = h.qs + h.al - 1u; te = h.tl + h.al - 1u;
    o.q_num_insert = o.q_base_insert = o.t_num_insert = o.t_base_insert = 0;
    for (uint32_t k = h.nxt; k != 0; k = ws[k - 1].nxt) {
      const K4BNode t = ws[k - 1];
      const int64_t qg = (int64_t)t.qs - (int64_t)qe - 1, tg = (int64_t)t.tl - (int64_t)te - 1;
      qe = t.qs + t.al - 1u; te = t.tl + t.al - 1u;
      if (qg > 0) { o.q_num_insert++; o.q_base_insert += (uint32_t)qg; }
      if (tg > 0) { o.t_num_insert++; o.t_base_insert += (uint32_t)tg; }
      nb++;
    }
    o.query = (uint32_t)q; o.targ_seq_id = h.tid; o.strand = h.flags & K4B_STRAND; o.score = h.score;
    o.q_start = h.qs; o.q_end = qe; o.t_start = h.tl; o.t_end = te; o.n_blocks = nb; o.block_off = 0;
  }
  __syncthreads();  // (the lanes read the blocks lane 0 has just settled)
  // BlocksAlignStats: a base above T on either side is an N and a mismatch
  uint32_t m = 0, x = 0, nn = 0;
  for (uint32_t k = head + 1u; k != 0; k = ws[k - 1].nxt) {
    const K4BNode t = ws[k - 1];
    for (uint32_t j = (uint32_t)lane; j < t.al; j += 64) {
      const uint32_t qb = sq.q(t.qs + j), tb = sq.t(t.tl + j);
      if ((qb & 7u) > 3u || (tb & 7u) > 3u) { nn++; x++; }
      else if (qb == tb) m++;
      else x++;
    }
  }
  m = k4d_wave_sum(m); x = k4d_wave_sum(x); nn = k4d_wave_sum(nn);
  if (lane == 0) {
    o.matches = m; o.mismatches = x; o.n_count = nn;
    const uint64_t at = path_offs[q] + r;
    out[at] = o;
    n_blocks[at] = nb;
  }
}

// the records where the caller wants them: block_off from the scan, the blocks of each path behind one another
__global__ void __launch_bounds__(64) k4k_blitz_emit(const K4BNode* __restrict__ ws, const uint32_t* __restrict__ sel, const uint32_t* __restrict__ cnt,
                                                     const uint64_t* __restrict__ path_offs, const uint64_t* __restrict__ block_offs, int64_t n,
                                                     int max_paths, const k4_blitz_path* __restrict__ in, k4_blitz_path* __restrict__ paths,
                                                     k4_blitz_block* __restrict__ blocks) {
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;  // a lane per (query, rank)
  const uint32_t r = blockIdx.y;
  if (q >= n || r >= cnt[q]) return;
  const uint64_t at = path_offs[q] + r;
  k4_blitz_path o = in[at];
  o.block_off = block_offs[at];
  paths[at] = o;
  uint64_t b = o.block_off;
  for (uint32_t k = sel[(uint64_t)q * (uint64_t)max_paths + r] + 1u; k != 0; k = ws[k - 1].nxt, b++) {
    k4_blitz_block bl;
    bl.len = ws[k - 1].al; bl.q_start = ws[k - 1].qs; bl.t_start = ws[k - 1].tl;
    blocks[b] = bl;
  }
}

// ==== host side ======================================================================================================
static int check_blitz_params(k4_index* ix, const k4_blitz_params* p) {
  if (!ix || !p) return K4_ERR_PARAMS;
  if (p->match_pts < 1 || p->match_pts > 10) return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: match_pts %d outside 1..10", p->match_pts);
  if (p->mismatch_pts < 1 || p->mismatch_pts > 10) return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: mismatch_pts %d outside 1..10", p->mismatch_pts);
  if (p->gap_open < 1 || p->gap_open > 50) return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: gap_open %d outside 1..50", p->gap_open);
  if (p->min_path_score < 0 || p->min_path_score > 100000)
    return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: min_path_score %d outside 0..100000", p->min_path_score);
  if (p->query_len_aligned_pct < 1 || p->query_len_aligned_pct > 100)
    return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: query_len_aligned_pct %d outside 1..100", p->query_len_aligned_pct);
  if (p->max_paths < 1 || p->max_paths > 10) return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: max_paths %d outside 1..10", p->max_paths);
  if (p->strand < 0 || p->strand > 2) return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: strand %d outside 0..2", p->strand);
  return K4_OK;
}

static unsigned bits_for(uint64_t v) {
  unsigned b = 0;
  while (v) { b++; v >>= 1; }
  return b;
}

extern "C" int k4_blitz_paths_batch_dev(k4_index* ix, const k4_blitz_params* p, int64_t n, const void* d_seqs, const void* d_offs,
                                        const void* d_lens, const void* d_node_offs, const void* d_nodes, void* d_path_offs, void* d_paths,
                                        uint64_t paths_cap, void* d_blocks, uint64_t blocks_cap, uint64_t* needed, void* stream) {
  int rc = check_blitz_params(ix, p);
  if (rc != K4_OK) return rc;
  K4BlitzState& b = ix->blz;
  b.timer.reset();
  if (n < 0 || n >= 0x7FFFFFFFll || !d_node_offs || !d_path_offs || !needed || (n > 0 && (!d_seqs || !d_offs || !d_lens)))
    return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: null argument");
  if ((paths_cap > 0 && !d_paths) || (blocks_cap > 0 && !d_blocks)) return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: a capacity without its buffer");
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  needed[0] = needed[1] = 0;
  uint64_t total = 0;
  K4_TRY(k4s_read_back(ix, &total, (const uint64_t*)d_node_offs + n, st));
  if (total >= 0xFFFFFFFEull) return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: at most 2^32-2 nodes per batch");
  if (total > 0 && !d_nodes) return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: null argument");
  const uint64_t max_sel = (uint64_t)n * (uint64_t)p->max_paths;
  K4_HIP(ix, b.cnt.reserve((size_t)(n + 1) * 4));
  K4_HIP(ix, b.offs.reserve((size_t)(n + 1) * 8));
  uint64_t* offs = b.offs.as<uint64_t>();
  uint64_t n_paths = 0, n_blocks = 0;
  if (total == 0) {  // no work: every query's paths start at 0
    K4_HIP(ix, hipMemsetAsync(offs, 0, (size_t)(n + 1) * 8, st));
  } else {
    K4_HIP(ix, b.timer.begin(st));
    for (K4DevBuf& kv : b.keys) K4_HIP(ix, kv.reserve((size_t)total * 8));
    for (K4DevBuf& kv : b.vals) K4_HIP(ix, kv.reserve((size_t)total * 4));
    K4_HIP(ix, b.qi.reserve((size_t)total * 4));
    K4_HIP(ix, b.nodes.reserve((size_t)total * sizeof(K4BNode)));
    K4_HIP(ix, b.list.reserve((size_t)total * 4 + 16));
    K4_HIP(ix, b.heads.reserve((size_t)total * 4 + 16));
    K4_HIP(ix, b.sel.reserve((size_t)std::max<uint64_t>(max_sel, 1) * 4));
    const k4_query_node* nodes = (const k4_query_node*)d_nodes;
    const uint64_t* node_offs = (const uint64_t*)d_node_offs;
    const unsigned nb = (unsigned)((total + 255) / 256);
    rocprim::double_buffer<uint64_t> keys(b.keys[0].as<uint64_t>(), b.keys[1].as<uint64_t>());
    rocprim::double_buffer<uint32_t> vals(b.vals[0].as<uint32_t>(), b.vals[1].as<uint32_t>());
    uint32_t* qi = b.qi.as<uint32_t>();
    K4BNode* ws = b.nodes.as<K4BNode>();
    hipLaunchKernelGGL(k4k_blitz_keys_lo, dim3(nb), dim3(256), 0, st, nodes, node_offs, n, total, keys.current(), vals.current(), qi);
    K4_TRY(k4s_sort_pairs<K4DevBuf>(ix, keys, vals, (size_t)total, 0, 64, st));
    hipLaunchKernelGGL(k4k_blitz_keys_hi, dim3(nb), dim3(256), 0, st, nodes, qi, vals.current(), total, keys.current());
    K4_TRY(k4s_sort_pairs<K4DevBuf>(ix, keys, vals, (size_t)total, 0, 33 + bits_for((uint64_t)n), st));
    hipLaunchKernelGGL(k4k_blitz_gather, dim3(nb), dim3(256), 0, st, nodes, qi, vals.current(), node_offs, total, ws);
    K4_HIP(ix, hipGetLastError());
    // the groups, one wave each per strand
    uint32_t* list = b.list.as<uint32_t>();
    uint64_t* d_m = reinterpret_cast<uint64_t*>(b.list.as<char>() + (((size_t)total * 4 + 7) & ~(size_t)7));
    uint64_t n_groups = 0;
    K4_TRY(k4s_select<K4DevBuf>(ix, rocprim::counting_iterator<uint32_t>(0), list, d_m, (size_t)total, K4BHasFlag{ws, K4B_GROUP}, st));
    K4_TRY(k4s_read_back(ix, &n_groups, d_m, st));
    K4BlitzArgs a;
    a.ix = ix->d;
    a.seqs = (const uint8_t*)d_seqs; a.offs = (const uint64_t*)d_offs; a.lens = (const uint32_t*)d_lens; a.node_offs = node_offs;
    a.n = n; a.p = *p; a.ws = ws; a.qi = qi; a.vals = vals.current(); a.total = total;
    hipLaunchKernelGGL(k4k_blitz_score, dim3((unsigned)n_groups, 2), dim3(64), 0, st, a, list, n_groups);
    K4_HIP(ix, hipGetLastError());
    // the heads, the first max_paths of each query, where each query's paths start
    uint32_t* heads = b.heads.as<uint32_t>();
    uint64_t* d_h = reinterpret_cast<uint64_t*>(b.heads.as<char>() + (((size_t)total * 4 + 7) & ~(size_t)7));
    uint64_t n_heads = 0;
    K4_TRY(k4s_select<K4DevBuf>(ix, rocprim::counting_iterator<uint32_t>(0), heads, d_h, (size_t)total, K4BHasFlag{ws, K4B_FIRST}, st));
    K4_TRY(k4s_read_back(ix, &n_heads, d_h, st));
    uint32_t* cnt = b.cnt.as<uint32_t>();
    uint32_t* sel = b.sel.as<uint32_t>();
    hipLaunchKernelGGL(k4k_blitz_pick, dim3((unsigned)(n + 1)), dim3(64), 0, st, ws, heads, n_heads, node_offs, n, (int)p->max_paths, sel, cnt);
    K4_HIP(ix, hipGetLastError());
    K4_TRY(k4s_exclusive_scan<K4DevBuf>(ix, cnt, offs, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
    K4_TRY(k4s_read_back(ix, &n_paths, offs + n, st));
    if (n_paths > 0) {
      K4_HIP(ix, b.paths.reserve((size_t)n_paths * sizeof(k4_blitz_path)));
      K4_HIP(ix, b.nb.reserve((size_t)(n_paths + 1) * 4));
      K4_HIP(ix, b.boffs.reserve((size_t)(n_paths + 1) * 8));
      uint32_t* nbk = b.nb.as<uint32_t>();
      uint64_t* boffs = b.boffs.as<uint64_t>();
      hipLaunchKernelGGL(k4k_blitz_path, dim3((unsigned)(n + 1), (unsigned)p->max_paths), dim3(64), 0, st, a, sel, cnt, offs,
                         b.paths.as<k4_blitz_path>(), nbk);
      K4_HIP(ix, hipGetLastError());
      K4_TRY(k4s_exclusive_scan<K4DevBuf>(ix, nbk, boffs, (uint64_t)0, (size_t)(n_paths + 1), rocprim::plus<uint64_t>(), st));
      K4_TRY(k4s_read_back(ix, &n_blocks, boffs + n_paths, st));
    }
  }
  needed[0] = n_paths;
  needed[1] = n_blocks;
  const bool fits = n_paths <= paths_cap && n_blocks <= blocks_cap;
  if (fits) {
    K4_HIP(ix, hipMemcpyAsync(d_path_offs, offs, (size_t)(n + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (n_paths > 0)
      hipLaunchKernelGGL(k4k_blitz_emit, dim3((unsigned)((n + 63) / 64), (unsigned)p->max_paths), dim3(64), 0, st, b.nodes.as<K4BNode>(),
                         b.sel.as<uint32_t>(), b.cnt.as<uint32_t>(), offs, b.boffs.as<uint64_t>(), n, (int)p->max_paths,
                         b.paths.as<k4_blitz_path>(), (k4_blitz_path*)d_paths, (k4_blitz_block*)d_blocks);
    K4_HIP(ix, hipGetLastError());
  }
  K4_HIP(ix, b.timer.end(st));
  K4_TRY(k4s_call_close(ix, st, b.timer));
  if (!fits)
    return k4_fail(ix, K4_ERR_MEM, "blitz paths: %llu paths and %llu blocks found, paths_cap is %llu and blocks_cap %llu", (unsigned long long)n_paths,
                   (unsigned long long)n_blocks, (unsigned long long)paths_cap, (unsigned long long)blocks_cap);
  return K4_OK;
}

extern "C" int k4_blitz_paths_batch(k4_index* ix, const k4_blitz_params* p, int64_t n, const uint8_t* seqs, const uint64_t* offs,
                                    const uint32_t* lens, const uint64_t* node_offs, const k4_query_node* nodes, uint64_t* path_offs,
                                    k4_blitz_path* paths, uint64_t paths_cap, k4_blitz_block* blocks, uint64_t blocks_cap, uint64_t* needed) {
  int rc = check_blitz_params(ix, p);
  if (rc != K4_OK) return rc;
  K4BlitzState& b = ix->blz;
  b.timer.reset();
  if (n < 0 || !node_offs || !path_offs || !needed || (n > 0 && (!seqs || !offs || !lens)) || (node_offs[n] > 0 && !nodes) ||
      (paths_cap > 0 && !paths) || (blocks_cap > 0 && !blocks))
    return k4_fail(ix, K4_ERR_PARAMS, "blitz paths: null argument");
  K4SeqStage& s = ix->seq_stage;
  const uint64_t total = node_offs[n];
  hipStream_t st;
  K4_TRY(k4s_call_open(ix, &st));
  K4_TRY(k4s_stage_seqs(ix, n, seqs, offs, lens, nullptr));
  K4_HIP(ix, s.node_offs.reserve((size_t)(n + 1) * 8));
  K4_HIP(ix, s.nodes.reserve((size_t)std::max<uint64_t>(total, 1) * sizeof(k4_query_node)));
  K4_HIP(ix, b.out_offs.reserve((size_t)(n + 1) * 8));
  K4_HIP(ix, b.out_paths.reserve((size_t)std::max<uint64_t>(paths_cap, 1) * sizeof(k4_blitz_path)));
  K4_HIP(ix, b.out_blocks.reserve((size_t)std::max<uint64_t>(blocks_cap, 1) * sizeof(k4_blitz_block)));
  K4_HIP(ix, hipMemcpyAsync(s.node_offs.p, node_offs, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
  if (total) K4_HIP(ix, hipMemcpyAsync(s.nodes.p, nodes, (size_t)total * sizeof(k4_query_node), hipMemcpyHostToDevice, st));
  rc = k4_blitz_paths_batch_dev(ix, p, n, s.seqs.p, s.offs.p, s.lens.p, s.node_offs.p, s.nodes.p, b.out_offs.p, b.out_paths.p, paths_cap,
                                b.out_blocks.p, blocks_cap, needed, st);
  if (rc != K4_OK) return rc;  // (nothing of the outputs has been written)
  K4_HIP(ix, hipMemcpyAsync(path_offs, b.out_offs.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
  if (needed[0]) K4_HIP(ix, hipMemcpyAsync(paths, b.out_paths.p, (size_t)needed[0] * sizeof(k4_blitz_path), hipMemcpyDeviceToHost, st));
  if (needed[1]) K4_HIP(ix, hipMemcpyAsync(blocks, b.out_blocks.p, (size_t)needed[1] * sizeof(k4_blitz_block), hipMemcpyDeviceToHost, st));
  return k4s_call_close(ix, st, b.timer);
}

extern "C" double k4_blitz_last_kernel_ms(const k4_index* ix) { return ix ? ix->blz.timer.ms : 0.0; }
