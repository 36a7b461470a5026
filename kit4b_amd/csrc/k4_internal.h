// kit4b_amd/csrc/k4_internal.h -- shared between the translation units of libk4sfx.so (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <thread>
#include <vector>
#include "../../include/k4sfx.h"
#include "k4_pool.h"

// ---- HBM layout of the index --------------------------------------------------------------------------
// ref2      2-bit packed reference, MSB-first inside 32-bit words: base i lives in bits (30 - 2*(i & 15)) of
//           word (i >> 4); non-ACGT symbols (N=4, EOS=7) are stored as 0 and described by the exception data.
//           K4_PAD_WORDS zero words sit in front of base 0 and behind the last base, so a window that starts up
//           to K4_PAD_BASES before 0 or runs past the end can be fetched without bounds tests.
// excbm     one bit per 256-base block (K4_EXC_SHIFT): set when the block holds a non-ACGT symbol.  1.5 MB for 3 Gbp,
//           so it lives in every XCD's L2; a read window spans at most a few blocks -> one 8-byte fetch per probe.
// excblk    sorted list of the flagged block numbers; excnib holds, for flagged block r, its 256 symbols as
//           nibbles (32 words, symbol j in bits 4*(j&7) of word r*32 + (j>>3)) -- the exact 4-bit reference.
// sa        the .sfx suffix array unchanged: 4- or 5-byte little-endian elements.
// ktab      direct-address table over the first k bases, 4^k + 1 entries {lb, pos0, sig} (12 bytes; 16 bytes when
//           concat_len >= 2^32: 64-bit lb, then 40-bit pos0 and a 12-base sig sharing a word): lb[c] = number of suffixes that sort before the k-mer with code c
//           (first base most significant), so the bucket of c is SA[lb[c] .. lb[c+1]); pos0[c] = SA[lb[c]], the
//           offset of the bucket's first suffix, which saves the dependent SA fetch for the first probe of a lookup;
//           sig[c] = the 16 bases after the k-mer in that suffix: a core that disagrees with it cannot match a
//           single-suffix bucket, so no probe is issued.
// entries   start/end offsets and ids of the chromosomes (tsSfxEntry), sorted by start.
#define K4_EXC_SHIFT 8            // log2 of the exception-bitmap block size in bases
#define K4_EXC_BLOCK (1 << K4_EXC_SHIFT)
#define K4_SUP_WORDS 512           // LDS-resident coarse exception bitmap: 16 Kbit, one bit per 2^sup_shift bases
#define K4_LDS_ENTRIES 128         // chromosome tables up to this size are searched in LDS
#define K4_PAD_BASES 2048
#define K4_PAD_WORDS (K4_PAD_BASES / 16)
#define K4_MAX_FAST_READ_LEN 512   // longer reads run in the general kernel
#define K4_MAX_READ_LEN 4096       // cMaxSeqLen is 2000 (KAligner.h:115)
#define K4_PROF_SLOTS 32          // u64 slots behind k4_counters for builds with -DK4_SLOW_PROF (tools/slow_prof.py)
#ifndef K4_DEEP_BUCKET
#define K4_DEEP_BUCKET 24          // k-mer table buckets deeper than this mark repeat families (k4_align.hip: K4_DEFER_BUCKET)
#endif
#define K4_DEDUP_CAP 6             // distinct candidates per strand pass kept by the fast kernel
#define K4_MAX_IDENT_NODES 1024000 // cMaxNumIdentNodes, libkit4b/SfxArray.h:15

struct K4DevIndex {
  const uint32_t* ref2;   // points at the word holding base 0
  const uint32_t* excbm;
  const uint32_t* excsup;  // K4_SUP_WORDS words: bit b set when bases [b << sup_shift, (b+1) << sup_shift) hold an exception
  const uint32_t* excblk;
  const uint32_t* excnib;
  const uint8_t* sa;
  const void* ktab;
  const uint64_t* ent_start;
  const uint64_t* ent_end;
  const uint32_t* ent_id;
  uint64_t n;        // ConcatSeqLen
  uint32_t n_exc;
  uint32_t n_entries;
  uint32_t el;       // 4 | 5
  uint32_t k;        // k-mer table length
  uint32_t ktab64;   // table entries are 64-bit
  uint32_t sup_shift; // log2 bases per bit of excsup (== K4_EXC_SHIFT when the whole fine bitmap fits)
  int32_t max_iter;
};

struct K4Workspace {
  int64_t cap_reads = 0;
  int32_t cap_len = 0;
  int32_t cap_hits = 0;
  K4DevBuf ids[2];       // survivors of a step: {read id, read length} (K4Survivor, 8 bytes; ids[1] also the deferred list's u32 ids) ...
  K4DevBuf rows[2];      // ... and their packed rows (u64, K4_ROW_WORDS a row: forward words and the two offset-0 memos)
  K4DevBuf slow_list;    // read ids (u32) for the general kernel
  K4DevBuf slow_step;    // and the phase ordinal (u8) at which each left the fast path
  K4DevBuf huge_list;    // reads that outgrew the small dedupe tables of the first general pass
  K4DevBuf huge_step;
  K4DevBuf ctl;          // u32, K4_CTL_WORDS (k4_align_common.h): [0] slow count, [1] slow head, [2+t] survivor count of step t,
                         // [68] [69] huge count / head, [70] deferred slots, [71] [72+t] tiles claimed in a launch
  K4DevBuf slow_hash;    // u64, per slow lane: open-addressing table of (generation<<32 | TargSeqID)
  uint32_t slow_hash_cap = 0;    // entries per lane (power of two)
  // staging for the host-pointer entry points
  K4DevBuf d_reads, d_offs, d_lens;
  K4DevBuf d_out4;       // rslt/inst/low/nxt or k4_read_result
  K4DevBuf d_hits;
  int64_t stage_reads = 0; int32_t stage_hits = 0;
  // small host-pointer batches (the facade's AlignReads groups): one pinned block up, one down.  [0, K4_SMALL_STAGE/2):
  // offs | lens | reads; [K4_SMALL_STAGE/2, K4_SMALL_STAGE): results | hits -- same layout in h_small and d_small
  uint8_t* h_small = nullptr;  // (pinned: k4_close frees it)
  K4DevBuf d_small;
  // where the current host-pointer batch lives on the device (d_small or the d_* buffers above)
  const uint8_t* c_reads = nullptr; const uint64_t* c_offs = nullptr; const uint32_t* c_lens = nullptr;
  int32_t* c_out = nullptr; k4_hit* c_hits = nullptr; bool c_small = false;
};

// The sequence batch of a host-pointer search call on the device (k4s_stage_seqs, k4_stage.h), grow-only: every family whose call
// takes sequences puts them here, LocateQuerySeqs and blitz's path stage also the node table that goes from one to the other
struct K4SeqStage { K4DevBuf seqs, offs, lens, node_offs, nodes; };
// LocateQuerySeqs (k4_query.hip), grow-only: per-query node slices and counts (cap_queries x cap_slice slots; the counts end with
// the zero the offsets' scan reads), the scan's temporary
struct K4QueryState {
  K4DevBuf ws, cnt;
  int64_t cap_queries = 0;
  uint64_t cap_slice = 0;
  K4Scratch<K4DevBuf> scan;
  K4Timer timer;
};
// blitz's path stage (k4_blitz.hip), grow-only: the sort's keys and values, the query of each node, the sorted nodes with their
// scores, the group and head lists, the chosen heads, per-query path counts and offsets, the path records with their block counts
// and offsets; then the outputs of the host-pointer entry point
struct K4BlitzState {
  K4DevBuf keys[2], vals[2], qi, nodes, list, heads, sel, cnt, offs, paths, nb, boffs;
  K4DevBuf out_offs, out_paths, out_blocks;
  K4Timer timer;
};
// restricted Hammings (k4_hamming.hip), grow-only: the span table of a batch, then the caller's byte array of the host-pointer forms
struct K4HammState { K4DevBuf spans, out; K4Timer timer; };
// K-mer cultivar counts (k4_cults.hip), grow-only and sized by the window and the entries, never by the range: a window's flags,
// entries and segment starts with the select's count, the count pass's answers and their scans, the histogram slices for indexes
// of more entries than the LDS histogram holds, the scans' temporary; then the outputs of the host-pointer entry point
struct K4CultState {
  K4DevBuf flags, ent, starts, count, loc, rep, nnz, loc_pre, rep_pre, dist_pre, hist;
  K4DevBuf out_kmers, out_bases, out_dist;
  K4Scratch<K4DevBuf> scan;
  K4Timer timer;  // (a section per window pass: the call reports their sum)
};

// kmarkers (k4_kmarkers.hip), grow-only: the rank of every entry in the target list, the outputs of the host-pointer entry points
// (status bytes; first indices and counts; MatchesOtherChroms answers), the four tallies and the long-run flag
struct K4MarkState { K4DevBuf rank, out, ctl; K4Timer timer; };
// genzygosity (k4_zygosity.hip), grow-only: the outputs and probe origins of the host-pointer entry points, the scan's internal
// status bytes and source-entry offsets, the list of probes that wait for the second launch, its dedupe tables, the control block
struct K4ZygState { K4DevBuf out, status, pre, list, big, ctl; K4Timer timer; uint64_t second = 0; };

struct k4_index {
  int device = 0;
  K4DevIndex d{};
  // the blocks d points into (ref2: K4_PAD_WORDS in front of d.ref2; sa: empty when d.sa is an array the caller lent, k4_open_device)
  K4DevBuf ref2, excbm, excsup, excblk, excnib, sa, ktab, ent_start, ent_end, ent_id;
  K4DevBuf counters;  // device k4_counters
  // FASTQ qualities (kalign -g, etFQMethod): 3 = ignored (the default); 0 Sanger / 1 Illumina 1.3+ / 2 Solexa: the parser puts the
  // scaled 4-bit score of every base into bits 4..7 of its read byte (the reference's own in-memory form), the SAM / BAM writers emit it
  int q_method = 3;
  K4DevBuf d_qlut;              // 256 bytes: quality character -> 4-bit score of the chosen method
  // `kalign -O` run tallies (k4_align_stats_collect, k4_stats.hip): K4_STATS_MULTI multihit bins, then K4_STATS_PE_LEN + 1 insert lengths;
  // empty = not collected (the align and pairing kernels then do nothing more than before)
  K4DevBuf d_run_stats;
  // `kalign -B`: the priority regions (k4_set_priority_regions, k4_priority.hip).  pri_off[c] .. pri_off[c + 1] are the intervals of
  // entry id c in pri_start / pri_end (sorted, disjoint, inclusive); pri_n = 0: no table, the align calls do what they did before
  // A feature of no bases (BED start == end) is kept as the reference keeps it, End = Start - 1: it meets every span that covers both
  // Start - 1 and Start.  Those sit apart, as sorted points: pri_pt_off[c] .. pri_pt_off[c + 1] in pri_pt.
  K4DevBuf pri_off, pri_start, pri_end, pri_pt_off, pri_pt;
  uint32_t pri_n = 0;    // intervals + points
  K4DevBuf pri_scratch[10];  // the priority pass's scratch (wide records and hits, marks, list, the normal call's inputs and records): grow-only
  double pri_ms[3] = {0, 0, 0};  // while kernel timing is on: the wide pass, the select kernel, the normal pass + scatter (host clock)
  uint64_t pri_reads[2] = {0, 0};  // reads that went through the priority pass / that needed the normal pass behind it
  uint64_t filter_prior[20] = {0};  // reads the filter stages (k4_filter.hip) marked so far, by the NAR they carried before
  double deep_bucket_frac = 0;  // share of the suffixes that sit in k-mer buckets deeper than K4_DEEP_BUCKET (k4_index.hip)
  std::vector<k4_entry> entries;
  std::string dataset;
  std::string description, title;  // header text for k4_write_sfx (k4_set_description)
  std::vector<uint8_t> raw_header;  // the file's tsSfxHeaderV3 when the index was opened from a .sfx
  uint64_t tot_seqs_len = 0;
  uint64_t device_bytes = 0;
  std::string err;
  K4Workspace ws;
  // paired-end pass (k4_pe.hip): both ends' SE results, their hit slots, the orphan list, {orphan count, error flag}
  K4DevBuf pe_rr, pe_hits, pe_list, pe_ctl;
  int64_t pe_cap_pairs = 0;
  int32_t pe_cap_hits = 0;
  // staging of k4_mate_rescue_batch (grow-only)
  K4DevBuf rs_tasks, rs_reads, rs_res, rs_hits;
  // the search-call families (DESIGN.md "Search-call families: shared scaffold"); their host-pointer forms share one staged batch
  K4SeqStage seq_stage;
  K4QueryState qry;
  K4BlitzState blz;
  K4HammState hmm;
  K4CultState cul;
  K4MarkState kmk;
  K4ZygState zyg;
  // k4_open_async: the arrays are uploaded and the device structures built by this thread; k4_open_wait joins it
  std::thread loader;
  int load_rc = 0;
  double load_seconds = 0;  // what that thread took
  hipStream_t stream = nullptr; // internal stream for the host-pointer entry points
  bool timing = false;          // bracket k4k_align_fast with events
  std::vector<hipEvent_t> ev0, ev1, ev2;  // before the step kernels, behind them, behind the general kernel's passes
  size_t ev_used = 0;
};

void k4_set_global_error(const char* fmt, ...);
int k4_fail(k4_index* ix, int code, const char* fmt, ...);
int k4_check_hip(k4_index* ix, hipError_t e, const char* what);

// k4_index.hip
int k4i_build_device_structures(k4_index* ix, const void* d_seq_bytes, int kmer_k);
const k4_entry* k4i_entry_by_id(const k4_index* ix, uint32_t entry_id);  // null when the table holds no such id
// k4_align.hip
#define K4_SMALL_STAGE (4u << 20)
#define K4_SMALL_READS 4096
int k4i_kalign_batch_dev(k4_index* ix, const k4_kalign_params* p, int64_t n, int32_t max_len, const void* d_reads,
                         const void* d_offs, const void* d_lens, void* d_out, void* d_hits, void* stream, int sparse_hits);
// the body of the k4_kalign_*_batch_dev calls without a priority table: the step kernels and the general kernel over n reads
int k4i_kalign_core(k4_index* ix, const k4_kalign_params* p, int64_t n, int32_t max_len, const void* d_reads, const void* d_offs,
                    const void* d_lens, void* d_out, void* d_hits, void* d_seg2, void* stream, int sparse_hits);
// k4_priority.hip: the same with a priority table set (CKAligner::ProcCoredApprox's priority pass in front of the normal one)
int k4i_priority_kalign(k4_index* ix, const k4_kalign_params* p, int64_t n, int32_t max_len, const void* d_reads, const void* d_offs,
                        const void* d_lens, void* d_out, void* d_hits, void* d_seg2, void* stream, int sparse_hits);
// k4_stats.hip: the run tallies of `kalign -O` (no-ops while k4_align_stats_collect is off)
int k4i_stats_tally_multi(k4_index* ix, const void* d_rr, int64_t n, void* stream);
unsigned long long* k4i_stats_pe_len_dist(k4_index* ix);
// k4_contam.hip: the table of `kalign -H` in HBM, per class (teContamType) its entries by falling length: bits = 12 rows
// (plane 0..2 x word 0..3 of k4_contaminant) of n[cls] words each, lens = n[cls] lengths; and k4_contam_trims_dev over it
struct K4ContamDev {
  K4DevBuf bits[4], lens[4];
  uint32_t n[4] = {0, 0, 0, 0};
};
int k4i_contam_upload(k4_index* ix, const k4_contaminant* tbl, int32_t n, K4ContamDev* out);
int k4i_contam_trims(k4_index* ix, const K4ContamDev& t, int pe, int64_t n_units, int32_t trim5, int32_t trim3, int32_t sample_nth,
                     int64_t first_unit, const void* d_reads, const void* d_offs1, const void* d_lens1, const void* d_offs2,
                     const void* d_lens2, uint64_t reads2_base, void* d_contam5, void* d_contam3, uint64_t* totals4, hipStream_t st);
// k4_sabuild.hip
int k4i_build_sa(uint64_t n, uint32_t el, const uint8_t* d_seq, uint8_t* d_sa, int device, std::string* err);

#define K4_HIP(ix, call)                                   \
  do {                                                     \
    int _rc = k4_check_hip((ix), (call), #call);           \
    if (_rc != K4_OK) return _rc;                          \
  } while (0)
