// kit4b_amd/csrc/k4_peinserts.hip -- `kalign -3` (--petranslendist): the PE insert length distribution of every target sequence,
// counted on the device over the pair records the align entry points and the global stages left in HBM, printed on the host:
//   k4_pe_insert_dist_dev    <- the walk of CKAligner::ReportPEInsertLenDist  ngskit4b/KAligner.cpp:5321-5454 over the order of
//                               CKAligner::SortPEHitMatch :10928-10963, and CKAligner::MedianInsertLen :5256-5319
//   k4_write_pe_insert_dist  <- its text (:5354-5357 the header, :5383-5386 / :5440-5443 a row)
//
// The reference sorts the reads that are accepted and PE-aligned to the front, by (ChromID of Seg[0], pair ordinal, PE1 before PE2),
// and walks them TWO AT A TIME: elements 2j and 2j + 1 are "pair j", on the target of element 2j, whether or not they are mates (a
// stage behind the pairing may have taken one mate out: every pairing behind it on that walk is shifted by one, a last odd element
// is dropped).  That is restated as it is.  Per target only the first K4_PEI_MAX_PAIRS pairs of the walk are counted.  Data-parallel:
//   1. select the accepted PE-aligned reads (ascending index = pair ordinal, PE1 before PE2) and sort them by target alone with a
//      stable radix sort over the bits target ids can reach (k4_stage.h): that is the walk order
//   2. select the pair slots whose target differs from the slot before: the row heads.  A target's run of slots starts at its head,
//      so a slot's rank in the run, the run's length and the compact row number all come from this list; nothing is sized by the
//      number of sequences of the index
//   3. k4k_pei_pairs, a thread per pair slot, every block over its own stretch of consecutive slots: TLen in the reference's 32-bit
//      unsigned arithmetic, the sort key (row, TLen) of a kept pair, and the 52 columns and the 64-bit sum of the block's CURRENT row
//      in LDS, added to the row's counters once, when the stretch leaves the row or ends.  A row that begins and ends inside one step
//      of 256 slots is touched by these threads alone and is short: its pairs are added to the row's counters directly.
//   4. sort the keys: a row's kept lengths ascending, the pairs behind the first million (length field all ones) last in their row
//   5. k4k_pei_rows, a thread per row: MedianInsertLen from the sorted lengths and the row's first one (k4_pe_insert_rule.h)
// The records are only read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#include "k4_device.h"
#include "k4_pe_insert_rule.h"
#include "k4_stage.h"

#define K4_PEI_ROW_W 56     // words of a row's device counters: [0, 52) the columns, [52] its first TLen, [53] unused, [54, 56) the 64-bit sum
#define K4_PEI_DROPPED 0xFFFFFFFFu

namespace {

struct IsPeAligned {  // NAR == eNARAccepted && FlgPEAligned (:10939, :5374)
  K4ReadSet s;
  __device__ bool operator()(uint32_t i) const {
    k4_hit h;
    return s.accepted(i, h) && s.pr[i].pe_aligned != 0;
  }
};

// the target of a selected read; an id no sequence has is kept apart in one value behind the last one, so that `bits` cover every key
__global__ void __launch_bounds__(256) k4k_pei_keys(const K4ReadSet s, uint32_t m, uint32_t n_entries, const uint32_t* __restrict__ idx,
                                                    uint32_t* __restrict__ key) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= m) return;
  key[k] = min(s.pr[idx[k]].hit.chrom_id, n_entries + 1u);
}

struct IsRowHead {  // pair slot j is on the target of element 2j (:5378)
  const uint32_t* key;
  __device__ bool operator()(uint32_t j) const { return j == 0 || key[2 * (size_t)j] != key[2 * (size_t)j - 2]; }
};

// the last head at or in front of slot j, among heads[lo .. n_rows) where heads[lo] <= j
__device__ __forceinline__ uint32_t row_of(const uint32_t* __restrict__ heads, uint32_t lo, uint32_t n_rows, uint32_t j) {
  uint32_t hi = n_rows;  // heads[hi] > j (or hi == n_rows)
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (heads[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) k4k_pei_pairs(const K4ReadSet s, uint32_t n_slots, uint32_t per_block, const uint32_t* __restrict__ idx,
                                                     const uint32_t* __restrict__ heads, uint32_t n_rows, uint32_t* __restrict__ acc,
                                                     uint64_t* __restrict__ tkey) {
  __shared__ uint32_t bins[K4_PEI_BINS];
  __shared__ unsigned long long row_sum;
  __shared__ uint32_t last_row[2];
  const uint64_t b0 = (uint64_t)blockIdx.x * per_block;
  if (b0 >= n_slots) return;
  const uint32_t j0 = (uint32_t)b0, j1 = b0 + per_block < n_slots ? (uint32_t)(b0 + per_block) : n_slots;
  if (threadIdx.x < K4_PEI_BINS) bins[threadIdx.x] = 0;
  if (threadIdx.x == K4_PEI_BINS) row_sum = 0;
  uint32_t cur = row_of(heads, 0, n_rows, j0);  // the row whose counters this block holds in LDS
  __syncthreads();
  // the pairs of the current row: the columns by LDS atomics, the lengths summed over the wave first
  auto add_current = [&](bool mine, uint32_t tlen) {
    if (mine) atomicAdd(&bins[k4_pei_bin(tlen)], 1u);
    unsigned long long v = mine ? tlen : 0u;
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&row_sum, v);
  };
  auto flush = [&](uint32_t row) {
    uint32_t* a = acc + (size_t)row * K4_PEI_ROW_W;
    if (threadIdx.x < K4_PEI_BINS && bins[threadIdx.x]) {
      atomicAdd(&a[threadIdx.x], bins[threadIdx.x]);
      bins[threadIdx.x] = 0;
    }
    if (threadIdx.x == K4_PEI_BINS && row_sum) {
      atomicAdd(reinterpret_cast<unsigned long long*>(a + 54), row_sum);
      row_sum = 0;
    }
  };
  uint32_t step = 0;
  for (uint32_t base = j0; base < j1; base += 256u, step++) {
    const uint32_t j = base + threadIdx.x;
    uint32_t row = cur, tlen = 0;
    bool keep = false;
    if (j < j1) {
      if (cur + 1u < n_rows && j >= heads[cur + 1u]) row = row_of(heads, cur + 1u, n_rows, j);
      const k4_hit h1 = s.pr[idx[2 * (size_t)j]].hit, h2 = s.pr[idx[2 * (size_t)j + 1]].hit;
      const uint32_t s1 = k4d_adj_start(h1) + 1u, s2 = k4d_adj_start(h2) + 1u;  // :5410-5417
      tlen = s1 <= s2 ? (s2 - s1) + k4d_adj_len(h2) : (s1 - s2) + k4d_adj_len(h1);
      const uint32_t rank = j - heads[row];
      keep = rank < K4_PEI_MAX_PAIRS;  // (:5404: a later pair is passed over altogether)
      tkey[j] = ((uint64_t)row << 32) | (keep ? tlen : K4_PEI_DROPPED);
      if (rank == 0) acc[(size_t)row * K4_PEI_ROW_W + 52] = tlen;
      if (j == j1 - 1u || threadIdx.x == 255u) last_row[step & 1u] = row;
    }
    __syncthreads();
    const uint32_t last = last_row[step & 1u];  // (the slot written two steps on lies behind the next step's barrier)
    if (keep && row != cur && row != last) {    // a row inside this step
      uint32_t* a = acc + (size_t)row * K4_PEI_ROW_W;
      atomicAdd(&a[k4_pei_bin(tlen)], 1u);
      atomicAdd(reinterpret_cast<unsigned long long*>(a + 54), (unsigned long long)tlen);
    }
    add_current(keep && row == cur, tlen);
    if (last != cur) {  // (the same for every thread of the block)
      __syncthreads();
      flush(cur);
      __syncthreads();
      cur = last;
      add_current(keep && row == cur, tlen);
    }
  }
  __syncthreads();
  flush(cur);
}

// per row: its target, how many pairs were counted, the median
__global__ void __launch_bounds__(256) k4k_pei_rows(uint32_t n_rows, uint32_t n_slots, const uint32_t* __restrict__ heads,
                                                    const uint32_t* __restrict__ key, const uint64_t* __restrict__ sorted,
                                                    const uint32_t* __restrict__ acc, uint32_t* __restrict__ out3) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n_rows) return;
  const uint32_t from = heads[r], to = r + 1u < n_rows ? heads[r + 1u] : n_slots;
  const uint32_t n = min(to - from, K4_PEI_MAX_PAIRS);
  const K4PeiSorted<2> vals = {reinterpret_cast<const uint32_t*>(sorted + from), n};  // (little endian: the length is a key's low word)
  out3[r] = key[2 * (size_t)from];
  out3[n_rows + r] = n;
  out3[2 * (size_t)n_rows + r] = k4_pei_median(vals, acc[(size_t)r * K4_PEI_ROW_W + 52]);
}

}  // namespace

extern "C" int k4_pe_insert_dist_dev(k4_index* ix, int64_t n_pairs, const void* d_pe, k4_pe_insert_dist* out, void* stream) {
  if (!ix || !out) return K4_ERR_PARAMS;
  memset(out, 0, sizeof(*out));
  if (n_pairs < 0 || n_pairs >= 0x7FFFFF80ll) return k4_fail(ix, K4_ERR_PARAMS, "pair count out of range (at most 2^31-128 pairs per call)");
  K4ReadSet s;
  K4_TRY(k4s_read_set(ix, 1, n_pairs, nullptr, nullptr, 0, d_pe, nullptr, nullptr, nullptr, nullptr, K4RS_UNITS, &s));
  K4_HIP(ix, hipSetDevice(ix->device));
  hipStream_t st = (hipStream_t)stream;
  auto host_block = [&](uint32_t n_rows) -> int {  // entry_id | tot_pes | median | dist[n_rows][52] (u32), then sum (u64)
    const size_t n32 = ((size_t)n_rows * (3 + K4_PEI_BINS) + 1) & ~(size_t)1;
    uint32_t* blk = (uint32_t*)calloc(n32 * 4 + (size_t)n_rows * 8 + 8, 1);
    if (!blk) return k4_fail(ix, K4_ERR_MEM, "out of memory");
    out->block = blk;
    out->n_rows = n_rows;
    out->entry_id = blk;
    out->tot_pes = blk + n_rows;
    out->median = blk + 2 * (size_t)n_rows;
    out->dist = blk + 3 * (size_t)n_rows;
    out->sum = (uint64_t*)(blk + n32);
    return K4_OK;
  };
  auto run = [&]() -> int {
    // 1. the walk order
    K4DevBuf idx0, idx1, key0, key1, heads, acc, tk0, tk1, rows;
    uint64_t m64 = 0;
    if (n_pairs > 0) K4_TRY(k4s_select_indices(ix, idx0, (size_t)s.n_reads, IsPeAligned{s}, st, &m64));
    else K4_HIP(ix, hipStreamSynchronize(st));
    const uint32_t m = (uint32_t)m64, n_slots = m / 2u;  // (:5370: a last odd element has no partner)
    if (n_slots == 0) return host_block(0);
    K4_HIP(ix, idx1.alloc((size_t)m * 4));
    K4_HIP(ix, key0.alloc((size_t)m * 4));
    K4_HIP(ix, key1.alloc((size_t)m * 4));
    hipLaunchKernelGGL(k4k_pei_keys, dim3((m + 255u) / 256u), dim3(256), 0, st, s, m, ix->d.n_entries, idx0.as<uint32_t>(), key0.as<uint32_t>());
    K4_HIP(ix, hipGetLastError());
    rocprim::double_buffer<uint32_t> kb(key0.as<uint32_t>(), key1.as<uint32_t>());
    rocprim::double_buffer<uint32_t> vb(idx0.as<uint32_t>(), idx1.as<uint32_t>());
    unsigned bits = 1;  // keys reach n_entries + 1
    while (bits < 32 && (((uint64_t)ix->d.n_entries + 1u) >> bits) != 0) bits++;
    K4_TRY(k4s_sort_pairs<K4DevBuf>(ix, kb, vb, (size_t)m, 0u, bits, st));
    // 2. the rows
    uint64_t r64 = 0;
    K4_TRY(k4s_select_indices(ix, heads, (size_t)n_slots, IsRowHead{kb.current()}, st, &r64));
    const uint32_t n_rows = (uint32_t)r64;
    K4_TRY(host_block(n_rows));
    // 3. the pairs
    K4_HIP(ix, acc.alloc((size_t)n_rows * K4_PEI_ROW_W * 4));
    K4_HIP(ix, hipMemsetAsync(acc.p, 0, (size_t)n_rows * K4_PEI_ROW_W * 4, st));
    K4_HIP(ix, tk0.alloc((size_t)n_slots * 8));
    K4_HIP(ix, tk1.alloc((size_t)n_slots * 8));
    const uint32_t steps = (n_slots + 255u) / 256u, blocks = std::min<uint32_t>(steps, 256u * 8u);
    const uint32_t per_block = (steps + blocks - 1u) / blocks * 256u;
    hipLaunchKernelGGL(k4k_pei_pairs, dim3(blocks), dim3(256), 0, st, s, n_slots, per_block, vb.current(), heads.as<uint32_t>(), n_rows,
                       acc.as<uint32_t>(), tk0.as<uint64_t>());
    K4_HIP(ix, hipGetLastError());
    // 4. 5. the medians
    rocprim::double_buffer<uint64_t> tb(tk0.as<uint64_t>(), tk1.as<uint64_t>());
    unsigned top = 33;
    while (top < 64 && (((uint64_t)n_rows - 1u) >> (top - 32)) != 0) top++;
    K4_TRY(k4s_sort_keys<K4DevBuf>(ix, tb, (size_t)n_slots, 0u, top, st));
    K4_HIP(ix, rows.alloc((size_t)n_rows * 3 * 4));
    hipLaunchKernelGGL(k4k_pei_rows, dim3((n_rows + 255u) / 256u), dim3(256), 0, st, n_rows, n_slots, heads.as<uint32_t>(), kb.current(),
                       tb.current(), acc.as<uint32_t>(), rows.as<uint32_t>());
    K4_HIP(ix, hipGetLastError());
    std::vector<uint32_t> a((size_t)n_rows * K4_PEI_ROW_W);
    K4_HIP(ix, hipMemcpyAsync(out->entry_id, rows.p, (size_t)n_rows * 3 * 4, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipMemcpyAsync(a.data(), acc.p, a.size() * 4, hipMemcpyDeviceToHost, st));
    K4_HIP(ix, hipStreamSynchronize(st));
    for (uint32_t r = 0; r < n_rows; r++) {
      const uint32_t* row = a.data() + (size_t)r * K4_PEI_ROW_W;
      memcpy(out->dist + (size_t)r * K4_PEI_BINS, row, K4_PEI_BINS * 4);
      memcpy(&out->sum[r], row + 54, 8);
    }
    return K4_OK;
  };
  const int rc = run();
  if (rc != K4_OK) k4_free_pe_insert_dist(out);
  return rc;
}

extern "C" void k4_free_pe_insert_dist(k4_pe_insert_dist* d) {
  if (!d) return;
  free(d->block);
  memset(d, 0, sizeof(*d));
}

extern "C" int k4_pe_insert_bin_host(uint32_t tlen) { return (int)k4_pei_bin(tlen); }

// values: a target's insert lengths in walk order (the order matters through values[0] alone)
extern "C" int k4_pe_insert_median_host(const uint32_t* values, uint32_t n, uint32_t* median) {
  if (!median || (!values && n)) return K4_ERR_PARAMS;
  std::vector<uint32_t> sorted(values, values + n);
  std::sort(sorted.begin(), sorted.end());
  *median = k4_pei_median(K4PeiSorted<1>{sorted.data(), n}, n ? values[0] : 0u);
  return K4_OK;
}

// The reference keeps the file open from before the reads load and leaves it empty when no read of the run was accepted
// (KAligner.cpp:771: the call sits inside `if (m_NARAccepted)`); else the header is written whether or not a pair was counted.
extern "C" int k4_write_pe_insert_dist(k4_index* ix, const k4_pe_insert_dist* d, uint64_t n_accepted, const char* path) {
  if (!ix || !d || !path || !path[0]) return K4_ERR_PARAMS;
  if (!d->block) return k4_fail(ix, K4_ERR_PARAMS, "k4_write_pe_insert_dist: the distributions were not filled (k4_pe_insert_dist_dev)");
  std::string o;
  if (n_accepted > 0) {
    char b[192];
    o += "\"TargSeq\",\"TargLen\",\"TotPEs\",\"MedianInsertLen\",\"MeanInsertLen\",\"Insert <100bp\"";
    for (int k = 0; k < 50; k++) o.append(b, (size_t)snprintf(b, sizeof(b), ",\"Insert %dbp\"", 100 + 10 * k));
    o += ",\"Insert >600bp\"\n";
    for (uint32_t r = 0; r < d->n_rows; r++) {
      const uint32_t id = d->entry_id[r];
      if (id < 1 || id > ix->entries.size()) return k4_fail(ix, K4_ERR_PARAMS, "k4_write_pe_insert_dist: row %u names sequence %u, which the index does not have", r, id);
      if (!d->tot_pes[r]) continue;
      const k4_entry& en = ix->entries[id - 1];
      o.append(b, (size_t)snprintf(b, sizeof(b), "\"%s\",%u,%u,%u,%u", en.name, en.seq_len, d->tot_pes[r], d->median[r],
                                   (uint32_t)(d->sum[r] / d->tot_pes[r])));
      for (int k = 0; k < K4_PEI_BINS; k++) o.append(b, (size_t)snprintf(b, sizeof(b), ",%u", d->dist[(size_t)r * K4_PEI_BINS + k]));
      o += "\n";
    }
  }
  FILE* fp = fopen(path, "wb");
  bool ok = fp && fwrite(o.data(), 1, o.size(), fp) == o.size();
  if (fp && fclose(fp) != 0) ok = false;
  if (!ok) return k4_fail(ix, K4_ERR_CREATE_FILE, "unable to write %s", path);
  return K4_OK;
}
