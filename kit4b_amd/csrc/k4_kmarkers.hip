// kit4b_amd/csrc/k4_kmarkers.hip -- `ngskit4b kmarkers` (ngskit4b/LocKMers.cpp: CLocKMers::LocateSpeciesUniqueKMers, :1085-1232) and the
// two CSfxArray calls it asks through, IterateExacts (libkit4b/SfxArray.cpp:3381-3458) and MatchesOtherChroms (:5094-5235), on gfx950.
//   k4k_exact_ranges     one LANE per probe: the run of suffixes that match it exactly (k4q_count, the search every family shares)
//   k4k_species_kmers    one WAVE per start locus of a target entry: the status the reference's single thread gives that K-mer.  The
//                        runs of the K-mer and of its reverse complement are walked 64 elements at a time; the reference's base flags
//                        become a minimum over (place in the target list, locus), so no wave waits for another and nothing is written
//                        into the index.  A survivor resolves the Hamming cores of both strands and the two prefixes one per lane.
//   k4k_matches_others   MatchesOtherChroms for a batch of probes, one wave each, over the same core walk
//   k4k_kmarkers_tally   the front end's four tallies from the status bytes
// DESIGN.md "kmarkers: the species scan" has the argument for the min-rank dedupe and the core walk.
#include <algorithm>
#include "k4_stage.h"

#define K4M_MAX_TARGETS 50      // cMaxTargCultivarChroms, LocKMers.h:26
#define K4M_MIN_KMER 20
#define K4M_MAX_KMER 100
#define K4M_MAX_PROBE 500       // MatchesOtherChroms probes (at CoreLen 8 that is 62 cores: one per lane)
#define K4M_MAX_RUN 0x7fffe     // an ACGT run of this many bases no longer fits a block of the front end (GetBlockSeqs, :454-474)
#define K4M_LAUNCH_KMERS 16384  // start loci (waves) per launch
#define K4M_SEEN_WORDS 64       // mode 2: the distinct entries of a prefix, one bit each
#define K4M_FOREIGN 0xFFu       // rank of an entry that is no target

enum { K4M_NOT_KMER = 1, K4M_FIRST_FOREIGN = 2, K4M_DUPLICATE = 3, K4M_FOREIGN_HIT = 4, K4M_HAMMING = 5, K4M_PREFIX = 6, K4M_ACCEPTED = 7 };

struct K4MTargets {
  uint64_t pre[K4M_MAX_TARGETS + 1];  // start loci of the targets in front, in processing order
  uint64_t start[K4M_MAX_TARGETS];    // concatenation offset of the target's first base
  uint32_t len[K4M_MAX_TARGETS];
  uint32_t n;
};

struct K4MScanArgs {
  K4DevIndex ix;
  K4MTargets t;
  const uint8_t* rank;  // per entry of the table: its place in the target list, K4M_FOREIGN for the others
  uint8_t* status;
  uint64_t k0, k1;      // this launch's start loci
  uint32_t K, min_hamming, core_len, n_core, prefix_len, min_with_prefix;
};

// MatchesOtherChroms (:5161-5235) by one wave, for the probe in pb on n_strands strands (1: as given; 2: then its reverse complement,
// the front end's second call): lane i resolves core i % n_core of strand i / n_core, then every run is walked by the whole wave.
// A core hit counts when its entry is not listed, the probe can be laid over it inside the entry (:5211-5216) -- and then the
// reference returns 1 whatever the flanks hold, its mismatch loop never being entered (NumMM > MaxTotMM is false at 0).
template <int EL>
K4_DEV bool k4m_matches_others(const K4DevIndex& ix, K4Tb& tb, const uint8_t* pb, uint32_t len, uint32_t core_len, uint32_t n_core,
                               int n_strands, const uint8_t* rank) {
  const int lane = threadIdx.x;
  const uint32_t n_items = n_core * (uint32_t)n_strands;
  uint64_t first;
  const uint32_t cnt = k4d_cores_to_lanes<EL>(
      ix, tb, lane, n_items, n_core, core_len, 0xFFFFFFFFu, [&](uint32_t s) { return K4QSeq{pb, len, (int)s}; },
      [&](uint32_t core) { return core * core_len; }, first);
  for (uint32_t it = 0; it < n_items; it++) {
    const uint32_t ofs = (it % n_core) * core_len;
    const bool hit = k4d_run_walk<EL>(ix, lane, __shfl(first, (int)it, 64), __shfl(cnt, (int)it, 64), [&](uint32_t, uint64_t pos, bool active) {
      if (!active) return false;
      const int e = k4d_map_entry(ix, pos);
      if (e < 0 || rank[e] != K4M_FOREIGN) return false;
      const uint32_t loci = (uint32_t)(pos - ix.ent_start[e]);
      const uint32_t seq_len = (uint32_t)(ix.ent_end[e] - ix.ent_start[e] + 1);
      return loci >= ofs && loci + len - ofs <= seq_len;  // (32-bit unsigned, as the reference computes it)
    });
    if (hit) return true;
  }
  return false;
}

// the entries outside the target list that hold an occurrence of the run [first, first + cnt), marked in seen; stops at `want`
// distinct entries (seen counts what earlier runs marked as well, :1169-1202).  Returns the count.
template <int EL>
K4_DEV uint32_t k4m_prefix_entries(const K4DevIndex& ix, uint64_t first, uint32_t cnt, const uint8_t* rank, uint32_t* seen, uint32_t have, uint32_t want) {
  const int lane = threadIdx.x;
  if (have >= want) return have;
  k4d_run_walk<EL>(ix, lane, first, cnt, [&](uint32_t, uint64_t pos, bool active) {
    const int e = active ? k4d_map_entry(ix, pos) : -1;
    if (e >= 0 && rank[e] == K4M_FOREIGN) atomicOr(&seen[e >> 5], 1u << (e & 31));
    __syncthreads();
    have = k4d_wave_sum((uint32_t)__popc(seen[lane]));
    __syncthreads();
    return have >= want;
  });
  return have;
}

template <int EL>
__global__ void __launch_bounds__(64) k4k_species_kmers(K4MScanArgs a) {
  __shared__ uint8_t pb[128];
  __shared__ uint32_t seen[K4M_SEEN_WORDS];
  const int lane = threadIdx.x;
  const uint64_t pid = a.k0 + blockIdx.x;
  if (pid >= a.k1) return;
  const uint32_t ti = k4d_last_le(a.t.n, pid, [&](uint32_t i) { return a.t.pre[i]; });  // the target that holds start locus pid
  const uint32_t locus = (uint32_t)(pid - a.t.pre[ti]), K = a.K;
  const uint64_t cpos = a.t.start[ti] + locus;
  const uint32_t rem = a.t.len[ti] - locus;
  K4Tb tb;
  tb.init(a.ix);
  // 1. K ACGT bases from here (:1085-1094)
  bool bad = false;
  for (uint32_t j = (uint32_t)lane; j < K; j += 64) {
    const uint32_t b = j < rem ? tb.get((int64_t)(cpos + j)) : 7u;
    pb[j] = (uint8_t)b;
    bad |= b > 3u;
  }
  seen[lane] = 0;
  const bool not_kmer = __ballot(bad) != 0;
  __syncthreads();
  if (not_kmer) {
    if (lane == 0) a.status[pid] = K4M_NOT_KMER;
    return;
  }
  // 2. the runs of the K-mer (lane 0) and of its reverse complement (lane 1)
  const auto strand = [&](uint32_t s) { return K4QSeq{pb, K, (int)s}; };
  const auto whole = [](uint32_t) { return 0u; };
  uint64_t first;
  uint32_t cnt = k4d_cores_to_lanes<EL>(a.ix, tb, lane, 2u, 1u, K, 0xFFFFFFFFu, strand, whole, first);
  const uint64_t fs = __shfl(first, 0, 64), fr = __shfl(first, 1, 64);
  const uint32_t cs = __shfl(cnt, 0, 64), cr = __shfl(cnt, 1, 64);
  // 3. :1105-1147.  The first sense hit decides between "foreign first hit" and the flags; a flag at the first hit of either strand
  // was set by an earlier occurrence, in processing order, of the K-mer, or of its reverse complement where that strand's first
  // hit lies in a target too (an occurrence whose own first hit is foreign sets nothing).  The walk behind the flags looks at every
  // sense hit, and at every antisense hit but the first (PrevHitIdx = RcplHitIdx, :1134).
  const uint64_t own = ((uint64_t)ti << 32) | locus;
  uint64_t min_key = ~0ull;
  bool foreign = false;
  const bool first_foreign = k4d_run_walk<EL>(a.ix, lane, fs, cs, [&](uint32_t i, uint64_t pos, bool active) {
    if (!active) return false;
    const int e = k4d_map_entry(a.ix, pos);
    const uint32_t r = e >= 0 ? a.rank[e] : K4M_FOREIGN;
    if (r != K4M_FOREIGN) min_key = min(min_key, ((uint64_t)r << 32) | (uint32_t)(pos - a.ix.ent_start[e]));
    else if (i > 0) foreign = true;
    return r == K4M_FOREIGN && i == 0;  // (the first hit: the walk ends in its first turn)
  });
  if (cs == 0 || first_foreign) {  // (cs == 0 cannot be: the K-mer stands at its own locus)
    if (lane == 0) a.status[pid] = K4M_FIRST_FOREIGN;
    return;
  }
  bool rc_first_target = false;
  k4d_run_walk<EL>(a.ix, lane, fr, cr, [&](uint32_t i, uint64_t pos, bool active) {
    uint32_t r = K4M_FOREIGN;
    uint64_t key = ~0ull;
    if (active) {
      const int e = k4d_map_entry(a.ix, pos);
      if (e >= 0) r = a.rank[e];
      if (r != K4M_FOREIGN) key = ((uint64_t)r << 32) | (uint32_t)(pos - a.ix.ent_start[e]);
      else if (i > 0) foreign = true;
    }
    if (i == (uint32_t)lane) rc_first_target = __shfl(r, 0, 64) != K4M_FOREIGN;  // (the first turn)
    if (rc_first_target) min_key = min(min_key, key);
    return false;
  });
  min_key = k4d_wave_min(min_key);
  // (a K-mer that is its own reverse complement finds the flag it has just set: SetBaseFlags with one locus twice)
  if ((cr > 0 && fr == fs) || min_key < own) {
    if (lane == 0) a.status[pid] = K4M_DUPLICATE;
    return;
  }
  if (__ballot(foreign)) {
    if (lane == 0) a.status[pid] = K4M_FOREIGN_HIT;
    return;
  }
  // 4. :1153-1159
  if (a.min_hamming > 1 && a.n_core > 0 && k4m_matches_others<EL>(a.ix, tb, pb, K, a.core_len, a.n_core, 2, a.rank)) {
    if (lane == 0) a.status[pid] = K4M_HAMMING;
    return;
  }
  // 5. :1167-1203
  if (a.prefix_len) {
    cnt = k4d_cores_to_lanes<EL>(a.ix, tb, lane, 2u, 1u, a.prefix_len, 0xFFFFFFFFu, strand, whole, first);
    uint32_t have = k4m_prefix_entries<EL>(a.ix, __shfl(first, 0, 64), __shfl(cnt, 0, 64), a.rank, seen, 0u, a.min_with_prefix);
    have = k4m_prefix_entries<EL>(a.ix, __shfl(first, 1, 64), __shfl(cnt, 1, 64), a.rank, seen, have, a.min_with_prefix);
    if (have < a.min_with_prefix) {
      if (lane == 0) a.status[pid] = K4M_PREFIX;
      return;
    }
  }
  if (lane == 0) a.status[pid] = K4M_ACCEPTED;
}

// NumKMers, NumPutativeKMers, NumAcceptedKMers, NumAcceptedExtdKMers (:1096, :1150, :1165, :1212 / :1220) from the status bytes.
// Mode 1 reports a run of adjacent accepted K-mers when a LATER accepted K-mer of the same ACGT run starts the next one (:1217-1222;
// the flush behind the loop, :1233, is mode 0's and finds nothing), so a run start counts when an accepted K-mer stands between it
// and the last status-1 byte in front: the K - 1 bytes that end every ACGT run and every target.
__global__ void __launch_bounds__(256) k4k_kmarkers_tally(const uint8_t* status, uint64_t n, int mode, unsigned long long* tot) {
  uint32_t c[4] = {0, 0, 0, 0};
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) {
    const uint32_t s = status[p];
    c[0] += s != K4M_NOT_KMER;
    c[1] += s >= K4M_HAMMING;
    c[2] += s >= K4M_PREFIX;
    if (s != K4M_ACCEPTED) continue;
    if (mode != 1) { c[3]++; continue; }
    if (p > 0 && status[p - 1] == K4M_ACCEPTED) continue;
    for (uint64_t q = p; q > 0; q--) {
      const uint32_t b = status[q - 1];
      if (b == K4M_NOT_KMER) break;
      if (b == K4M_ACCEPTED) { c[3]++; break; }
    }
  }
  k4d_tally_flush(c, tot);
}

// is an ACGT run of K4M_MAX_RUN bases or more in a target?  Such a run covers a locus that is a multiple of K4M_MAX_RUN / 2; one
// lane per such locus measures the run around it.
__global__ void __launch_bounds__(64) k4k_kmarkers_long_runs(K4DevIndex ix, K4MTargets t, unsigned long long* flag) {
  const uint32_t step = K4M_MAX_RUN / 2;
  K4Tb tb;
  tb.init(ix);
  for (uint32_t ti = blockIdx.x; ti < t.n; ti += gridDim.x)
    for (uint32_t l = step * ((uint32_t)threadIdx.x + 1); l < t.len[ti]; l += step * 64) {
      if (tb.get((int64_t)(t.start[ti] + l)) > 3u) continue;
      uint32_t run = 1;
      for (uint32_t q = l; q > 0 && run < K4M_MAX_RUN && tb.get((int64_t)(t.start[ti] + q - 1)) <= 3u; q--) run++;
      for (uint32_t q = l + 1; q < t.len[ti] && run < K4M_MAX_RUN && tb.get((int64_t)(t.start[ti] + q)) <= 3u; q++) run++;
      if (run >= K4M_MAX_RUN) atomicAdd(flag, 1ull);
    }
}

template <int EL>
__global__ void __launch_bounds__(64) k4k_exact_ranges(K4DevIndex ix, int64_t n, const uint8_t* seqs, const uint64_t* offs, const uint32_t* lens,
                                                       uint64_t* firsts, uint32_t* counts) {
  K4Tb tb;
  tb.init(ix);
  for (int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 64) {
    K4QSeq qs;
    qs.q = seqs + offs[i]; qs.len = lens[i]; qs.s = 0;
    uint64_t first = 0;
    const uint32_t cnt = qs.len ? k4q_count<EL>(ix, tb, qs, 0u, (int)qs.len, 0xFFFFFFFFu, first) : 0u;
    firsts[i] = cnt ? first : 0;
    counts[i] = cnt;
  }
}

template <int EL>
__global__ void __launch_bounds__(64) k4k_matches_others(K4DevIndex ix, int64_t n, const uint8_t* seqs, const uint64_t* offs, const uint32_t* lens,
                                                         const uint8_t* rank, uint32_t max_tot_mm, int32_t* out) {
  __shared__ uint8_t pb[512];
  const int lane = threadIdx.x;
  K4Tb tb;
  tb.init(ix);
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t len = lens[i];
    __syncthreads();  // (the probe before has been read)
    for (uint32_t j = (uint32_t)lane; j < len; j += 64) pb[j] = seqs[offs[i] + j] & 0x0fu;
    __syncthreads();
    const uint32_t core_len = max(8u, len / (1u + max_tot_mm));  // :5189-5192
    const uint32_t n_core = len > core_len ? (len - core_len + core_len - 1) / core_len : 0u;  // offsets 0, CoreLen, .. < len - CoreLen
    const bool m = n_core > 0 && k4m_matches_others<EL>(ix, tb, pb, len, core_len, n_core, 1, rank);
    if (lane == 0) out[i] = m ? 1 : 0;
  }
}

// ==== host side ======================================================================================================
// the rank table of a list of entry ids on the device; ids the index does not hold are passed over (MatchesOtherChroms compares ids)
static int kmarkers_rank(k4_index* ix, int n_ids, const uint32_t* ids, hipStream_t st, std::vector<uint8_t>& h_rank) {
  K4MarkState& m = ix->kmk;
  h_rank.assign((size_t)ix->d.n_entries, K4M_FOREIGN);
  for (int i = 0; i < n_ids; i++) {
    const k4_entry* e = k4i_entry_by_id(ix, ids[i]);
    if (e && h_rank[(size_t)(e - ix->entries.data())] == K4M_FOREIGN) h_rank[(size_t)(e - ix->entries.data())] = (uint8_t)i;
  }
  K4_HIP(ix, hipStreamSynchronize(st));  // (a table about to be replaced may still be read by the batch before)
  K4_HIP(ix, m.rank.reserve(h_rank.size() + 16));
  K4_HIP(ix, hipMemcpyAsync(m.rank.p, h_rank.data(), h_rank.size(), hipMemcpyHostToDevice, st));
  return K4_OK;
}

static int check_probes(k4_index* ix, const char* who, int64_t n, const void* seqs, const void* offs, const void* lens, const void* out) {
  if (!ix) return K4_ERR_PARAMS;
  ix->kmk.timer.reset();
  if (n < 0 || (n > 0 && (!seqs || !offs || !lens || !out))) return k4_fail(ix, K4_ERR_PARAMS, "%s: null argument", who);
  return K4_OK;
}

static int exact_ranges_run(k4_index* ix, int64_t n, const uint8_t* d_seqs, const uint64_t* d_offs, const uint32_t* d_lens, uint64_t* d_firsts,
                            uint32_t* d_counts, hipStream_t st) {
  K4MarkState& m = ix->kmk;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 63) / 64, 1 << 16);
  K4_HIP(ix, m.timer.begin(st));
  K4S_LAUNCH_EL(ix, k4k_exact_ranges, grid, 64, st, ix->d, n, d_seqs, d_offs, d_lens, d_firsts, d_counts);
  K4_HIP(ix, hipGetLastError());
  K4_HIP(ix, m.timer.end(st));
  return K4_OK;
}

extern "C" int k4_exact_ranges_batch_dev(k4_index* ix, int64_t n, const void* d_seqs, const void* d_offs, const void* d_lens, void* d_firsts,
                                         void* d_counts, void* stream) {
  int rc = check_probes(ix, "exact ranges", n, d_seqs, d_offs, d_lens, d_firsts);
  if (rc != K4_OK) return rc;
  if (n > 0 && !d_counts) return k4_fail(ix, K4_ERR_PARAMS, "exact ranges: null argument");
  if (n == 0) return K4_OK;
  K4_HIP(ix, hipSetDevice(ix->device));
  const hipStream_t st = (hipStream_t)stream;
  K4_TRY(exact_ranges_run(ix, n, (const uint8_t*)d_seqs, (const uint64_t*)d_offs, (const uint32_t*)d_lens, (uint64_t*)d_firsts, (uint32_t*)d_counts, st));
  return k4s_call_close(ix, st, ix->kmk.timer);
}

extern "C" int k4_exact_ranges_batch(k4_index* ix, int64_t n, const uint8_t* seqs, const uint64_t* offs, const uint32_t* lens, uint64_t* firsts,
                                     uint32_t* counts) {
  int rc = check_probes(ix, "exact ranges", n, seqs, offs, lens, firsts);
  if (rc != K4_OK) return rc;
  if (n > 0 && !counts) return k4_fail(ix, K4_ERR_PARAMS, "exact ranges: null argument");
  if (n == 0) return K4_OK;
  K4MarkState& m = ix->kmk;
  hipStream_t st;
  K4_TRY(k4s_call_open(ix, &st));
  K4_TRY(k4s_stage_seqs(ix, n, seqs, offs, lens, nullptr));
  K4_HIP(ix, m.out.reserve((size_t)n * 12 + 16));
  uint64_t* d_firsts = m.out.as<uint64_t>();
  uint32_t* d_counts = (uint32_t*)(d_firsts + n);
  K4_TRY(exact_ranges_run(ix, n, ix->seq_stage.seqs.as<uint8_t>(), ix->seq_stage.offs.as<uint64_t>(), ix->seq_stage.lens.as<uint32_t>(), d_firsts,
                          d_counts, st));
  K4_HIP(ix, hipMemcpyAsync(firsts, d_firsts, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  K4_HIP(ix, hipMemcpyAsync(counts, d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  return k4s_call_close(ix, st, m.timer);
}

extern "C" int k4_matches_other_chroms_batch(k4_index* ix, int32_t n_ids, const uint32_t* ids, int32_t max_tot_mm, int64_t n, const uint8_t* seqs,
                                             const uint64_t* offs, const uint32_t* lens, int32_t* matches) {
  int rc = check_probes(ix, "MatchesOtherChroms", n, seqs, offs, lens, matches);
  if (rc != K4_OK) return rc;
  if (n_ids < 0 || n_ids > K4M_MAX_TARGETS || (n_ids > 0 && !ids) || max_tot_mm < 0)
    return k4_fail(ix, K4_ERR_PARAMS, "MatchesOtherChroms: %d ids (0..%d) or MaxTotMM %d below 0", n_ids, K4M_MAX_TARGETS, max_tot_mm);
  for (int64_t i = 0; i < n; i++)
    if (lens[i] > K4M_MAX_PROBE) return k4_fail(ix, K4_ERR_PARAMS, "MatchesOtherChroms: probe %lld of %u bases, at most %d", (long long)i, lens[i], K4M_MAX_PROBE);
  if (n == 0) return K4_OK;
  K4MarkState& m = ix->kmk;
  hipStream_t st;
  K4_TRY(k4s_call_open(ix, &st));
  std::vector<uint8_t> h_rank;
  K4_TRY(kmarkers_rank(ix, n_ids, ids, st, h_rank));
  K4_TRY(k4s_stage_seqs(ix, n, seqs, offs, lens, nullptr));
  K4_HIP(ix, m.out.reserve((size_t)n * 4 + 16));
  const unsigned grid = (unsigned)std::min<int64_t>(n, 1 << 16);
  K4_HIP(ix, m.timer.begin(st));
  K4S_LAUNCH_EL(ix, k4k_matches_others, grid, 64, st, ix->d, n, ix->seq_stage.seqs.as<uint8_t>(), ix->seq_stage.offs.as<uint64_t>(),
                ix->seq_stage.lens.as<uint32_t>(), m.rank.as<uint8_t>(), (uint32_t)max_tot_mm, m.out.as<int32_t>());
  K4_HIP(ix, hipGetLastError());
  K4_HIP(ix, m.timer.end(st));
  K4_HIP(ix, hipMemcpyAsync(matches, m.out.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  return k4s_call_close(ix, st, m.timer);
}

// the species scan on a device status array, its arguments checked; *total = the status bytes written
static int species_run(k4_index* ix, const k4_kmarkers_params* p, int32_t n_targets, const uint32_t* target_ids, uint8_t* d_status, uint64_t status_len,
                       bool on_host, k4_kmarkers_totals* tot, uint64_t* total, hipStream_t st) {
  if (!ix) return K4_ERR_PARAMS;
  K4MarkState& m = ix->kmk;
  m.timer.reset();
  if (!p || !target_ids || !d_status || !tot) return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: null argument");
  if (p->kmer_len < K4M_MIN_KMER || p->kmer_len > K4M_MAX_KMER)
    return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: kmer_len %d outside %d..%d", p->kmer_len, K4M_MIN_KMER, K4M_MAX_KMER);
  if (p->min_hamming < 1 || p->min_hamming > 5) return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: min_hamming %d outside 1..5", p->min_hamming);
  if (p->mode < 0 || p->mode > 2) return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: mode %d outside 0..2", p->mode);
  if (p->mode == 2 && (p->prefix_len < K4M_MIN_KMER / 2 || p->prefix_len > p->kmer_len - K4M_MIN_KMER / 2))
    return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: prefix_len %d outside %d..%d", p->prefix_len, K4M_MIN_KMER / 2, p->kmer_len - K4M_MIN_KMER / 2);
  if (p->mode == 2 && p->min_with_prefix < 0) return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: min_with_prefix %d below 0", p->min_with_prefix);
  if (n_targets < 1 || n_targets > K4M_MAX_TARGETS) return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: %d targets, 1..%d", n_targets, K4M_MAX_TARGETS);
  if ((uint32_t)n_targets >= ix->d.n_entries)
    return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: %d targets leave none of the %u entries to compare with", n_targets, ix->d.n_entries);
  if (p->mode == 2 && ix->d.n_entries > K4M_SEEN_WORDS * 32)
    return k4_fail(ix, K4_ERR_UNSUPPORTED, "kmarkers: mode 2 over %u entries, at most %d", ix->d.n_entries, K4M_SEEN_WORDS * 32);
  K4MScanArgs a;
  a.t.n = (uint32_t)n_targets;
  a.t.pre[0] = 0;
  for (int i = 0; i < n_targets; i++) {
    const k4_entry* e = k4i_entry_by_id(ix, target_ids[i]);
    if (!e) return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: no entry with id %u", target_ids[i]);
    for (int j = 0; j < i; j++)
      if (target_ids[j] == target_ids[i]) return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: entry id %u twice in the target list", target_ids[i]);
    a.t.start[i] = e->start_ofs;
    a.t.len[i] = e->seq_len;
    a.t.pre[i + 1] = a.t.pre[i] + e->seq_len;
  }
  for (int i = n_targets; i < K4M_MAX_TARGETS; i++) { a.t.start[i] = 0; a.t.len[i] = 0; a.t.pre[i + 1] = a.t.pre[n_targets]; }
  *total = a.t.pre[n_targets];
  if (status_len < *total)
    return k4_fail(ix, K4_ERR_PARAMS, "kmarkers: %llu status bytes, the targets have %llu loci", (unsigned long long)status_len, (unsigned long long)*total);
  tot->processed = tot->cultivar_specific = tot->hamming_retained = tot->accepted = 0;
  if (*total == 0) return K4_OK;
  K4_HIP(ix, hipSetDevice(ix->device));
  std::vector<uint8_t> h_rank;
  K4_TRY(kmarkers_rank(ix, n_targets, target_ids, st, h_rank));
  K4_HIP(ix, m.ctl.reserve(8 * 8));
  K4_HIP(ix, hipMemsetAsync(m.ctl.p, 0, 8 * 8, st));
  unsigned long long* d_ctl = m.ctl.as<unsigned long long>();
  bool long_entry = false;
  for (int i = 0; i < n_targets; i++) long_entry |= a.t.len[i] >= K4M_MAX_RUN;
  if (long_entry) {
    unsigned long long n_long = 0;
    hipLaunchKernelGGL(k4k_kmarkers_long_runs, dim3((unsigned)n_targets), dim3(64), 0, st, ix->d, a.t, d_ctl + 4);
    K4_HIP(ix, hipGetLastError());
    K4_TRY(k4s_read_back(ix, &n_long, d_ctl + 4, st));
    if (n_long)
      return k4_fail(ix, K4_ERR_UNSUPPORTED, "kmarkers: a target holds a run of %d ACGT bases or more, which the reference's front end cannot block", K4M_MAX_RUN);
  }
  if (on_host) {
    K4_HIP(ix, m.out.reserve((size_t)*total + 16));
    d_status = m.out.as<uint8_t>();
  }
  a.ix = ix->d;
  a.rank = m.rank.as<uint8_t>();
  a.status = d_status;
  a.K = (uint32_t)p->kmer_len;
  a.min_hamming = (uint32_t)p->min_hamming;
  a.core_len = std::max<uint32_t>(8u, a.K / a.min_hamming);  // MaxTotMM = MinHamming - 1, :5189-5192
  a.n_core = a.K > a.core_len ? (a.K - a.core_len + a.core_len - 1) / a.core_len : 0u;
  a.prefix_len = p->mode == 2 ? (uint32_t)p->prefix_len : 0u;
  const uint32_t others = ix->d.n_entries - (uint32_t)n_targets;  // :719-720
  a.min_with_prefix = p->min_with_prefix == 0 || (uint32_t)p->min_with_prefix > others ? others : (uint32_t)p->min_with_prefix;
  K4_HIP(ix, m.timer.begin(st));
  k4s_launch_windows(*total, K4M_LAUNCH_KMERS, [&](uint64_t k0, uint64_t k1) {
    a.k0 = k0;
    a.k1 = k1;
    K4S_LAUNCH_EL(ix, k4k_species_kmers, (unsigned)(k1 - k0), 64, st, a);
  });
  hipLaunchKernelGGL(k4k_kmarkers_tally, dim3((unsigned)std::min<uint64_t>((*total + 255) / 256, 1024)), dim3(256), 0, st, d_status, *total, (int)p->mode, d_ctl);
  K4_HIP(ix, hipGetLastError());
  K4_HIP(ix, m.timer.end(st));
  unsigned long long t4[4] = {0, 0, 0, 0};
  K4_HIP(ix, hipMemcpyAsync(t4, d_ctl, sizeof(t4), hipMemcpyDeviceToHost, st));
  K4_TRY(k4s_call_close(ix, st, m.timer));
  tot->processed = t4[0]; tot->cultivar_specific = t4[1]; tot->hamming_retained = t4[2]; tot->accepted = t4[3];
  return K4_OK;
}

extern "C" int k4_species_kmers_batch_dev(k4_index* ix, const k4_kmarkers_params* p, int32_t n_targets, const uint32_t* target_ids, void* d_status,
                                          uint64_t status_len, k4_kmarkers_totals* totals, void* stream) {
  uint64_t total = 0;
  return species_run(ix, p, n_targets, target_ids, (uint8_t*)d_status, status_len, false, totals, &total, (hipStream_t)stream);
}

// host status array: the bytes of the targets' loci come back, the bytes behind them stay as they were
extern "C" int k4_species_kmers_batch(k4_index* ix, const k4_kmarkers_params* p, int32_t n_targets, const uint32_t* target_ids, uint8_t* status,
                                      uint64_t status_len, k4_kmarkers_totals* totals) {
  if (!ix) return K4_ERR_PARAMS;
  uint64_t total = 0;
  hipStream_t st;
  K4_TRY(k4s_call_open(ix, &st));
  const int rc = species_run(ix, p, n_targets, target_ids, status, status_len, true, totals, &total, st);
  if (rc != K4_OK || total == 0) return rc;
  K4_HIP(ix, hipMemcpyAsync(status, ix->kmk.out.p, (size_t)total, hipMemcpyDeviceToHost, st));
  return k4s_call_close(ix, st, ix->kmk.timer);
}

extern "C" double k4_kmarkers_last_kernel_ms(const k4_index* ix) { return ix ? ix->kmk.timer.ms : 0.0; }
