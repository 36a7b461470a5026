/* include/k4sfx.h -- C ABI of libk4sfx.so: the MI355X-native replacement for the kit4b kalign hot path
 * (seed lookup in the CSfxArray suffix-array index + mismatch-bounded full-read extension).
 *
 * The reference has no FFI layer: the boundary it exposes for this path is the C++ class CSfxArray
 * (libkit4b/SfxArray.h:524-1023) as called by CKAligner (ngskit4b/KAligner.cpp).  Each entry point below
 * names the reference method(s) it replaces.  Plain pointers and sizes only; no torch / HIP types.
 * The C++ facade that keeps the CSfxArray method names on top of this ABI is include/k4_sfxarray.hpp;
 * the binding a kit4b maintainer would add is shown in INTEGRATION.md.
 *
 * Result conventions (same as the reference):
 *   < 0          teBSFrsltCodes  (libkit4b/ErrorCodes.h:15-97), text via k4_last_error()
 *   0..4         tHRslt          (libkit4b/SfxArray.h:79-87) for per-read alignment results
 * There is NO CPU fallback: every compute entry point runs hand-written HIP kernels on gfx950 and fails
 * with K4_ERR_NO_DEVICE when no GPU is usable.
 */
#ifndef K4SFX_H
#define K4SFX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define K4_ABI_VERSION 2  /* 2: optional AlignReads phases (k4_hit.ext, k4_seg2, *_ext entry points), pipeline, comm */

/* teBSFrsltCodes values used by this library (libkit4b/ErrorCodes.h:15-97) */
enum {
  K4_OK = 0,               /* eBSFSuccess */
  K4_ERR_PARAMS = -100,    /* eBSFerrParams */
  K4_ERR_MEM = -95,        /* eBSFerrMem */
  K4_ERR_NOT_SFX = -94,    /* eBSFerrNotBioseq */
  K4_ERR_NOT_FASTA = -93,  /* eBSFerrNotFasta */
  K4_ERR_OPEN_FILE = -90,  /* eBSFerrOpnFile */
  K4_ERR_CREATE_FILE = -89,/* eBSFerrCreateFile */
  K4_ERR_FILE_VER = -86,   /* eBSFerrFileVer */
  K4_ERR_FILE_ACCESS = -85,/* eBSFerrFileAccess */
  K4_ERR_ENTRY = -51,      /* eBSFerrEntry */
  K4_ERR_PARSE = -47,      /* eBSFerrParse */
  K4_ERR_INTERNAL = -1,    /* eBSFerrInternal */
  K4_ERR_NO_DEVICE = -2,   /* (new) no usable gfx950 device / HIP runtime error */
  K4_ERR_UNSUPPORTED = -3  /* (new) feature outside the hot-path scope (bisulfite, colourspace, ...) */
};

/* tHRslt, libkit4b/SfxArray.h:79-87 */
enum { K4_HR_NONE = 0, K4_HR_HITS = 1, K4_HR_MMDELTA = 2, K4_HR_HITINSTS = 3, K4_HR_RMMDELTA = 4,
       K4_HR_SEQERRS = 5, K4_HR_FATAL = 6 };
/* eALStrand, libkit4b/SfxArray.h:72-77 */
enum { K4_STRAND_BOTH = 0, K4_STRAND_WATSON = 1, K4_STRAND_CRICK = 2 };
/* eNAR values AlignRead can assign, ngskit4b/KAligner.h:136-158 */
enum { K4_NAR_UNALIGNED = 0, K4_NAR_ACCEPTED = 1, K4_NAR_NS = 2, K4_NAR_NOHIT = 3, K4_NAR_MMDELTA = 4,
       K4_NAR_MULTIALIGN = 5, K4_NAR_TRIM = 6, K4_NAR_SPLICEJCTN = 7, K4_NAR_MICROINDEL = 8,
       K4_NAR_PCRDUP = 9 /* eNARPCRdup: removed as a potential PCR artefact (k4_reduce_pcr_dups_dev) */ };

typedef struct k4_index k4_index; /* opaque: the HBM-resident index (replaces a loaded CSfxArray) */

/* One tsHitLoci (libkit4b/SfxArray.h:239-260): Seg[0] as the default path fills it at SfxArray.cpp:6264-6307, plus -- in
 * `ext` -- what the optional phases of AlignReads add: Seg[0].TrimLeft / TrimRight and the Flg* bits.  16 bytes; `ext` is 0
 * on the default path.  The second segment of a microInDel / splice-junction hit lives in a k4_seg2 record. */
typedef struct {
  uint32_t chrom_id;   /* Seg[0].ChromID: 1-based tsSfxEntry.EntryID */
  uint32_t match_loci; /* Seg[0].MatchLoci: 0-based in the chromosome (the reference truncates to uint32) */
  uint16_t match_len;  /* Seg[0].MatchLen: the probe length; the first segment's length in a two-segment hit */
  uint8_t strand;      /* Seg[0].Strand: '+' or '-' */
  uint8_t mismatches;  /* Seg[0].Mismatches == Seg[0].TrimMismatches */
  uint32_t ext;        /* bits 0-11 Seg[0].TrimLeft, 12-23 Seg[0].TrimRight, then K4_EXT_* */
} k4_hit;
#define K4_EXT_CHIMERIC (1u << 24)  /* FlgChimeric: flank-trimmed alignment (`-c`, SfxArray.cpp:6064-6189) */
#define K4_EXT_INDEL (1u << 25)     /* FlgInDel: two segments around a microInDel (`-a`, :7526) */
#define K4_EXT_INSERT (1u << 26)    /* FlgInsert: the InDel is an insertion into the read */
#define K4_EXT_SPLICE (1u << 27)    /* FlgSplice: two segments around a splice junction (`-A`, :7208) */
#define K4_EXT_NONORPHAN (1u << 28) /* FlgNonOrphan: another read shares the junction (KAligner.cpp:2456-2465) */
#define K4_HIT_TRIM_LEFT(h) ((h).ext & 0xFFFu)
#define K4_HIT_TRIM_RIGHT(h) (((h).ext >> 12) & 0xFFFu)

/* Seg[1] of a two-segment hit and tsHitLoci.Score; one record per READ (LocateInDels / LocateSpliceJuncts report at most
 * one hit).  All zero unless hit slot 0 carries K4_EXT_INDEL or K4_EXT_SPLICE.  16 bytes. */
typedef struct {
  uint32_t chrom_id;   /* Seg[1].ChromID */
  uint32_t match_loci; /* Seg[1].MatchLoci */
  uint16_t match_len;  /* Seg[1].MatchLen */
  uint16_t read_ofs;   /* Seg[1].ReadOfs */
  uint8_t mismatches;  /* Seg[1].Mismatches */
  uint8_t reserved;
  uint16_t score;      /* Score */
} k4_seg2;

/* tsSfxEntry (libkit4b/SfxArray.h:98-106) without packing */
typedef struct {
  uint32_t entry_id;
  uint32_t fblock_id;
  char name[81];
  uint16_t name_hash;
  uint32_t seq_len;
  uint64_t start_ofs;
  uint64_t end_ofs;
} k4_entry;

typedef struct {
  uint64_t concat_len;   /* tsSfxBlock.ConcatSeqLen */
  uint64_t tot_seqs_len; /* CSfxArray::GetTotSeqsLen, SfxArray.h:970 */
  uint32_t sfx_el_size;  /* 4 | 5 */
  uint32_t n_entries;    /* CSfxArray::GetNumEntries, SfxArray.h:958 */
  uint32_t kmer_k;       /* length of the direct-address k-mer -> SA-interval table */
  uint32_t n_exc_blocks; /* 64-base blocks holding a non-ACGT symbol (N / EOS) */
  uint64_t device_bytes; /* HBM held by this index */
  int32_t device;        /* HIP device ordinal */
  int32_t max_iter;      /* CSfxArray::GetMaxIter */
  char dataset[81];      /* CSfxArray::GetDatasetName */
} k4_info_t;

/* The arguments of CSfxArray::AlignReads (libkit4b/SfxArray.h:614-634). */
typedef struct {
  int32_t tot_mm;          /* TotMM */
  int32_t core_len;        /* CoreLen */
  int32_t core_delta;      /* CoreDelta */
  int32_t max_core_slides; /* MaxNumCoreSlides */
  int32_t min_core_len;    /* MinCoreLen (used by the chimeric phase only, SfxArray.cpp:7925) */
  int32_t mm_delta;        /* MMDelta */
  int32_t strand;          /* Align2Strand: K4_STRAND_* */
  int32_t max_hits;        /* MaxHits */
  /* the optional phases a read enters when the ones above found nothing (SfxArray.cpp:7894-7930); 0 = off */
  int32_t min_chimeric_len;     /* MinChimericLen: 15..99, % of the read that must survive flank trimming */
  int32_t micro_indel_len;      /* microInDelLen: 1..20; needs the *_ext entry points (k4_seg2 output) */
  int32_t max_splice_junct_len; /* MaxSpliceJunctLen: 25..100000; needs the *_ext entry points */
} k4_align_params;

/* What CKAligner::AlignRead derives per read and how it classifies (ngskit4b/KAligner.cpp:9583-10105) */
typedef struct {
  int32_t max_subs;       /* -s per 100 bp (pPars->MaxSubs) */
  int32_t min_edit_dist;  /* -e (pPars->MinEditDist) 1|2 */
  int32_t max_ns;         /* -n (m_MaxNs), default 1 */
  int32_t pmode;          /* -m 0 default,1 more,2 ultra,3 less sensitive (KAligner.cpp:9377-9393) */
  int32_t strand;         /* K4_STRAND_* */
  int32_t max_ml;         /* max(m_MaxMLmatches, PE ? cMaxMLPEmatches : 0) (KAligner.cpp:9604) */
  int32_t pe_mode;        /* classification of a read with hits (KAligner.cpp:9907-10023): 0 SE, default MLMode (accepted,
                           * first instance); 1 PE (accepted iff one instance, else multi-aligned with NumHits = instances);
                           * 2 SE, MLMode eMLall (`-r5 -R<max_ml>`): accepted with NumHits = instances, every one reported;
                           * 3 = 2 with reads over the limit treated as if exactly max_ml matched (`-X`, :9856-9861);
                           * 4 = 3 through CSfxArray::LocateBestMatches (`-N`, SfxArray.cpp:6836-7205) instead of AlignReads */
  int32_t min_core_len;   /* 0: derive as LocateCoredApprox does (KAligner.cpp:9367-9393) */
  int32_t max_num_slides; /* 0: derive from pmode */
  int32_t min_chimeric_len;     /* -c (pPars->MinChimericLen, KAligner.cpp:9801): 0 or 15..99 */
  int32_t micro_indel_len;      /* -a (pPars->microInDelLen): 0..20; SE only; needs the *_ext entry points */
  int32_t max_splice_junct_len; /* -A (pPars->SpliceJunctLen): 0 or 25..100000; SE only; needs the *_ext entry points */
} k4_kalign_params;

typedef struct {
  int32_t hit_rslt; /* tHRslt from AlignReads (K4_HR_SEQERRS when the read has too many Ns) */
  int32_t inst;     /* tsReadHit.LowHitInstances */
  int32_t low_mm;   /* tsReadHit.LowMMCnt */
  int32_t nxt_mm;   /* tsReadHit.NxtLowMMCnt */
  int32_t nar;      /* tsReadHit.NAR */
  int32_t num_hits; /* tsReadHit.NumHits */
} k4_read_result;

/* run-time tallies for the roofline accounting; cumulative until k4_reset_counters */
typedef struct {
  uint64_t n_reads;    /* reads processed */
  uint64_t n_lookup;   /* seed lookups (one per LocateFirstExact the reference would have made) */
  uint64_t n_probe;    /* suffix-array probes actually issued (SA element + packed-reference window) */
  uint64_t n_cand;     /* candidates that reached the Hamming extension */
  uint64_t n_slow;     /* reads routed to the exact general kernel (N, separators, many candidates) */
  uint64_t n_bases;    /* read bases in */
} k4_counters;

/* ---- index life cycle ------------------------------------------------------------------------------
 * k4_open               <- CSfxArray::Open(path) + SetTargBlock(1)   SfxArray.h:528,957 (SfxArray.cpp:969,1982)
 * k4_open_host          <- same, from an in-memory block (CSfxArray::Open(bBisulfite,bColorspace) in-memory mode, SfxArray.h:533)
 * k4_open_device        <- same, adopting a 1-byte/base sequence and a suffix array already resident in HBM
 * k4_close              <- CSfxArray::Close/Reset                    SfxArray.h:527,548
 * kmer_k: 0 = choose from the index size; device: HIP ordinal. */
int k4_open(const char* sfx_path, int device, int kmer_k, k4_index** out);
/* k4_open in two halves (the reading of the reads can run beside the index load, as kalign's loader runs beside its aligner threads,
 * KAligner.cpp:4786-4866): k4_open_async returns once header and entry table are read; k4_info / k4_get_entry / k4_min_core_len /
 * k4_set_max_iter / k4_set_fastq_quality and a pipeline's ingest side (k4_pipeline_open, acquire / submit) may be used at once, a
 * library thread uploads the arrays and builds the device structures meanwhile.  k4_open_wait joins it and returns the load's
 * result; the pipeline waits by itself before its first alignment batch, every other entry point needs k4_open_wait first.
 * On an error from k4_open_wait the handle is still to be released with k4_close. */
int k4_open_async(const char* sfx_path, int device, int kmer_k, k4_index** out);
int k4_open_wait(k4_index* ix);
double k4_open_seconds(const k4_index* ix);  /* wall seconds the background load took (after k4_open_wait) */
int k4_open_host(uint64_t concat_len, uint32_t sfx_el_size, const uint8_t* seq, const uint8_t* sa,
                 uint32_t n_entries, const k4_entry* entries, const char* dataset, int device, int kmer_k,
                 k4_index** out);
int k4_open_device(uint64_t concat_len, uint32_t sfx_el_size, const void* d_seq, void* d_sa, int adopt_sa,
                   uint32_t n_entries, const k4_entry* entries, const char* dataset, int device, int kmer_k,
                   k4_index** out);
void k4_close(k4_index* ix);
/* k4_sfx_map / k4_sfx_unmap <- CSfxArray::Disk2Hdr / Disk2Entries (SfxArray.cpp:629-825): the .sfx file mapped read-only with
 * its tables decoded, for callers that place the index themselves (k4_open_host, or libk4comm's broadcast over xGMI) */
typedef struct {
  const void* map; size_t map_len;      /* the mapping (owned; k4_sfx_unmap releases it and `entries`) */
  uint64_t concat_len; uint32_t sfx_el_size, n_entries;
  k4_entry* entries;
  const uint8_t* seq;                   /* concat_len bytes, one etSeqBase per base, EOS separators */
  const uint8_t* sa;                    /* concat_len * sfx_el_size bytes */
  const uint8_t* header;                /* tsSfxHeaderV3, 1224 bytes */
  char dataset[81];
} k4_sfx_file;
int k4_sfx_map(const char* sfx_path, k4_sfx_file* out);
void k4_sfx_unmap(k4_sfx_file* f);
int k4_set_raw_header(k4_index* ix, const void* hdr_1224); /* the header an index opened from parts reports / writes */
const char* k4_last_error(const k4_index* ix);            /* <- CErrorCodes::GetErrMsg, ErrorCodes.h:99-113 */
const char* k4_global_error(void);                        /* error text when no index handle exists yet */
int k4_info(const k4_index* ix, k4_info_t* out);          /* <- GetNumEntries/GetTotSeqsLen/GetSfxHeader */
int k4_get_entry(const k4_index* ix, uint32_t entry_id, k4_entry* out); /* <- GetIdentName/GetSeqLen, SfxArray.h:967-969 */
int k4_get_ident(const k4_index* ix, const char* name);   /* <- CSfxArray::GetIdent, SfxArray.h:968 */
int k4_set_max_iter(k4_index* ix, int max_iter);          /* <- CSfxArray::SetMaxIter, SfxArray.h:556 */
/* k4_set_fastq_quality <- kalign -g<n> (etFQMethod, KAlignerCL.cpp:241,499): how the quality line of a FASTQ record is read --
 * 0 Sanger (Illumina 1.8+), 1 Illumina 1.3+, 2 Solexa / Illumina before 1.3, 3 ignore (the default).  With 0..2 k4_parse_fastx_dev
 * (and the pipeline) scale every base's score to 4 bits as LoadRawReads does (KAligner.cpp:12096-12158: phred clamped to 40,
 * (phred + 2) * 15 / 40) into bits 4..7 of the read byte, and the SAM / BAM writers report it as ReportBAMread does
 * (KAligner.cpp:6120-6145: '!' + score * 40 / 15, reversed for a Crick alignment, `*` / 0xff when every score is zero). */
int k4_set_fastq_quality(k4_index* ix, int method);
int k4_get_seq(const k4_index* ix, uint32_t entry_id, uint32_t loci, uint8_t* out, uint32_t len); /* <- GetSeq, SfxArray.h:996 */
int k4_write_sfx(const k4_index* ix, const char* sfx_path); /* <- CSfxArray::Finalise/Flush2Disk, SfxArray.cpp:892 */
int k4_set_description(k4_index* ix, const char* description, const char* title); /* <- SetDescription / SetTitle, SfxArray.h:552-553 */
int k4_get_sfx_header(const k4_index* ix, void* out_1224);  /* <- CSfxArray::GetSfxHeader: tsSfxHeaderV3, SfxArray.h:194-207 */

/* ---- suffix-array construction on the GPU -----------------------------------
 * <- CSfxArray::AddEntry + Finalise -> QSortSeq (SfxArray.cpp:1518,1758,9739): same suffix order
 * (A<C<G<T<N<EOS, compare stops after the first EOS), ties broken by offset.
 * d_seq: concat_len bytes in HBM (bases + one EOS per entry); d_sa: concat_len*sfx_el_size bytes in HBM, filled. */
int k4_build_sa_device(uint64_t concat_len, uint32_t sfx_el_size, const void* d_seq, void* d_sa, int device);

/* ---- the hot path -------------------------------------------------------------------------------------
 * k4_align_reads_batch  <- CSfxArray::AlignReads for n_reads fresh reads (In/Out ints start at 0 as in
 *                          KAligner.cpp:9609-9611,9678-9680), uniform parameters.   SfxArray.h:614 (SfxArray.cpp:7838)
 * k4_kalign_batch       <- CKAligner::AlignRead for n_reads reads.                  KAligner.cpp:9583
 * reads: concatenated etSeqBase bytes (A0 C1 G2 T3 N4; bits 3..7 ignored); read i = reads[offs[i] .. offs[i]+lens[i]).
 * hits: n_reads * max_hits records; slots beyond min(inst,max_hits) are zero.
 * *_dev variants take DEVICE pointers for every array and a hipStream_t (as void*); they enqueue only
 * (no host synchronisation) once the workspace has been sized by k4_reserve(). */
int k4_reserve(k4_index* ix, int64_t max_reads, int32_t max_read_len, int32_t max_hits);
int k4_align_reads_batch(k4_index* ix, const k4_align_params* p, int64_t n_reads, const uint8_t* reads,
                         const uint64_t* offs, const uint32_t* lens, int32_t* rslt, int32_t* inst, int32_t* low,
                         int32_t* nxt, k4_hit* hits);
int k4_align_reads_batch_dev(k4_index* ix, const k4_align_params* p, int64_t n_reads, int32_t max_read_len,
                             const void* d_reads, const void* d_offs, const void* d_lens, void* d_rslt, void* d_inst,
                             void* d_low, void* d_nxt, void* d_hits, void* stream);
int k4_kalign_batch(k4_index* ix, const k4_kalign_params* p, int64_t n_reads, const uint8_t* reads,
                    const uint64_t* offs, const uint32_t* lens, k4_read_result* out, k4_hit* hits);
int k4_kalign_batch_dev(k4_index* ix, const k4_kalign_params* p, int64_t n_reads, int32_t max_read_len,
                        const void* d_reads, const void* d_offs, const void* d_lens, void* d_out, void* d_hits,
                        void* stream);
int k4_min_core_len(const k4_index* ix, int pmode, int* max_num_slides); /* <- LocateCoredApprox, KAligner.cpp:9367-9393 */
/* The same two calls with the k4_seg2 output the microInDel / splice phases need: seg2 holds n_reads
 * records.  <- CSfxArray::AlignReads incl. LocateInDels (SfxArray.cpp:7526), LocateSpliceJuncts (:7208) and the chimeric
 * LocateCoreMultiples pass (:6064-6189, AdaptiveTrim :5561); <- CKAligner::AlignRead with -c / -a / -A. */
int k4_align_reads_ext_batch(k4_index* ix, const k4_align_params* p, int64_t n_reads, const uint8_t* reads,
                             const uint64_t* offs, const uint32_t* lens, int32_t* rslt, int32_t* inst, int32_t* low,
                             int32_t* nxt, k4_hit* hits, k4_seg2* seg2);
int k4_align_reads_ext_batch_dev(k4_index* ix, const k4_align_params* p, int64_t n_reads, int32_t max_read_len,
                                 const void* d_reads, const void* d_offs, const void* d_lens, void* d_rslt, void* d_inst,
                                 void* d_low, void* d_nxt, void* d_hits, void* d_seg2, void* stream);
int k4_kalign_ext_batch(k4_index* ix, const k4_kalign_params* p, int64_t n_reads, const uint8_t* reads,
                        const uint64_t* offs, const uint32_t* lens, k4_read_result* out, k4_hit* hits, k4_seg2* seg2);
int k4_kalign_ext_batch_dev(k4_index* ix, const k4_kalign_params* p, int64_t n_reads, int32_t max_read_len,
                            const void* d_reads, const void* d_offs, const void* d_lens, void* d_out, void* d_hits,
                            void* d_seg2, void* stream);
/* The post-alignment stages `kalign -A / -a / -x` run on the SE results (device arrays as k4_kalign_ext_batch_dev left them):
 * k4_auto_trim_flanks_dev     <- CKAligner::AutoTrimFlanks (KAligner.cpp:1714-1917): trims the flanks of one-segment hits
 *                                back to min_flank_exacts exactly matching bases (TrimLeft / TrimRight in k4_hit.ext); a read
 *                                that cannot keep half its length becomes K4_NAR_TRIM.  pe: the PE variant (no elimination).
 * k4_remove_orphan_juncts_dev <- RemoveOrphanSpliceJuncts / RemoveOrphanMicroInDels (KAligner.cpp:2406-2594), which =
 *                                K4_EXT_SPLICE or K4_EXT_INDEL: a junction no other read shares (within 3 bp at both ends)
 *                                loses its alignment (K4_NAR_SPLICEJCTN / K4_NAR_MICROINDEL).
 * Both wait for `stream` and return counts. */
int k4_auto_trim_flanks_dev(k4_index* ix, int32_t min_flank_exacts, int pe, int64_t n_reads, int32_t max_ml, void* d_rr,
                            void* d_hits, const void* d_reads, const void* d_offs, const void* d_lens, int64_t* n_eliminated,
                            void* stream);
int k4_remove_orphan_juncts_dev(k4_index* ix, uint32_t which, int64_t n_reads, int32_t max_ml, void* d_rr, void* d_hits,
                                const void* d_seg2, int64_t* n_removed, void* stream);
/* k4_reduce_pcr_dups_dev <- CKAligner::ReducePCRduplicates (KAligner.cpp:2303-2400; `kalign -k <win_len>`, 0..250, SE only):
 *                           for each accepted read's (chrom, AdjStartLoci, AdjHitLen, strand) stack, ranked by low_mm then load
 *                           order, the reads behind the stack's limit become K4_NAR_PCRDUP with num_hits = inst = 0.  The limit is
 *                           1..50 by the distinct same-strand start sites within win_len up- or downstream (NumUpUniques /
 *                           NumDnUniques), 0 for win_len 0.  Waits for `stream` and returns the count in *n_dups. */
int k4_reduce_pcr_dups_dev(k4_index* ix, int32_t win_len, int64_t n_reads, int32_t max_ml, void* d_rr, void* d_hits, int64_t* n_dups,
                           void* stream);
/* k4_pcr5_primer_correct_dev <- CKAligner::PCR5PrimerCorrect (KAligner.cpp:2115-2226; `kalign -6 <n>`, which aligns with
 *                           min(MaxSubs + n, 15) substitutions per 100 bp, :245-248, and calls this with the user's MaxSubs behind
 *                           ReducePCRduplicates and in front of AutoTrimFlanks, :642-651; SE and PE, genpba too): for each accepted
 *                           one-segment read whose match_len is the read's length and whose low_mm exceeds (max_subs * len + 50) / 100,
 *                           the bases among its first klen that differ from the target's (the window reverse complemented for a Crick
 *                           alignment; symbol codes compared, so an N on either side differs) are rewritten in d_reads to the target's
 *                           symbol, bits 3..7 of the byte kept, in read order until the read is within that bound; low_mm and the
 *                           hit's mismatches become the bound.  A read the klen bases cannot bring there becomes K4_NAR_NOHIT with
 *                           num_hits = 0, its bases and inst as they were.  klen: 1..12, kalign always passes 12; klen < 1 does nothing.
 *                           pe: d_rr_or_pe holds n_reads k4_pe_read records (both ends, read by read; d_hits unused), else
 *                           k4_read_result with hit slot 0 of d_hits.  Waits for `stream`; counts = reads corrected, bases corrected,
 *                           reads rejected.  A second call changes nothing. */
int k4_pcr5_primer_correct_dev(k4_index* ix, int32_t max_subs, int32_t klen, int pe, int64_t n_reads, int32_t max_ml, void* d_rr_or_pe,
                               void* d_hits, void* d_reads, const void* d_offs, const void* d_lens,
                               int64_t counts[3] /* reads corrected, bases corrected, reads rejected */, void* stream);
/* ---- which accepted alignments are kept (`kalign -5 <file>`, `-Z <regex>`, `-z <regex>`; kit4b_amd/csrc/k4_filter.hip) ------------
 * k4_filter_loci_constraints_dev <- CKAligner::IdentifyConstraintViolations (KAligner.cpp:2716-2765; AcceptLociConstraints :2647-2714,
 *                           AcceptBaseConstraint :2598-2645), which kalign runs behind ProcessPairedEnds / AssignMultiMatches and in front
 *                           of ReducePCRduplicates: an accepted read on a constrained sequence one of whose loci -- AdjStartLoci ..
 *                           AdjEndLoci of Seg[0], and of Seg[1] of a two-segment read (d_seg2, may be NULL) -- lies inside a constraint
 *                           that the read's base there (reverse complemented for a Crick alignment) does not satisfy becomes
 *                           K4_NAR_LOCICONSTRAINED with num_hits = inst = 0.  pe: n_units pairs in d_pe (d_rr, d_hits, d_seg2 unused), the
 *                           mate of such a read is marked with it whatever its own state, and counted; else n_units reads in d_rr and hit
 *                           slot 0 of d_hits.  constraints: HOST array, any order, at most 6400 over at most 64 sequences
 *                           (KAligner.h:92-93), 0 <= start <= end < the sequence's length.  Waits for `stream`; *n_removed = reads marked.
 * k4_filter_chroms_dev   <- CKAligner::FiltByChroms (:4025-4091), which kalign runs behind the flank autotrim and the orphan junction /
 *                           microInDel filters: an accepted read (slot 0) on a sequence whose byte in d_accept is 0 becomes
 *                           K4_NAR_CHROMFILT with num_hits = inst = 0.  d_accept: DEVICE array of n_entries + 1 bytes indexed by entry id.
 *                           pe: d_rr_or_pe holds n_reads k4_pe_read records (read by read, as the reference does), else k4_read_result.
 * k4_load_loci_constraints <- CKAligner::LoadLociConstraints (:1363-1545): a CSV of `sequence,start,end,bases` (0-based inclusive loci; bases
 *                           from ACGT, and R = "the target's base"), an optional title line, blank lines and # comments sloughed.  *tbl is
 *                           malloc'd (k4_free_host) and sorted by (sequence, start, end).  A line the reference turns down gives
 *                           K4_ERR_PARSE (a file that cannot be read K4_ERR_OPEN_FILE) with the reference's message in k4_last_error and,
 *                           when errbuf is not NULL, in errbuf (256 bytes).  Host only.
 * k4_chrom_accept_mask   <- CUtility::CompileREs / MatchExcludeRegExpr / MatchIncludeRegExpr (libkit4b/Utility.cpp:78-287) over every
 *                           sequence of the index: std::regex (ECMAScript) searched in the name up to its first blank; a sequence is kept
 *                           (mask[entry id] = 1) when no exclude expression matches and an include expression does, or none was given.
 *                           At most 20 of either kind (KAligner.h:33-34), each cut to 100 characters, blanks and one pair of quotes around it dropped; an expression
 *                           that does not compile gives K4_ERR_PARAMS.  mask: host, n_entries + 1 bytes.  Host only. */
typedef struct {
  uint32_t chrom_id;   /* tsConstraintLoci.ChromID: 1-based entry id */
  uint32_t start, end; /* StartLoci, EndLoci: 0-based, inclusive */
  uint8_t bits;        /* Constraint: 0x01 A, 0x02 C, 0x04 G, 0x08 T, 0x10 R (the read's base equals the target's) */
  uint8_t reserved[3];
} k4_loci_constraint;
int k4_filter_loci_constraints_dev(k4_index* ix, const k4_loci_constraint* constraints, int32_t n_constraints, int pe, int64_t n_units,
                                   int32_t max_ml, void* d_rr, const void* d_hits, const void* d_seg2, void* d_pe, const void* d_reads,
                                   const void* d_offs, const void* d_lens, int64_t* n_removed, void* stream);
int k4_filter_chroms_dev(k4_index* ix, const void* d_accept, int pe, int64_t n_reads, int32_t max_ml, void* d_rr_or_pe, const void* d_hits,
                         int64_t* n_removed, void* stream);
/* the reads the two calls above marked on this index so far, by the NAR they carried before (20 slots).  kalign prints its EN line from
 * a tally made while the reads are aligned (m_NumSloughedNs, KAligner.cpp:3732), so a PE mate that went from EN to LC is still in it. */
int k4_filter_marked_prior(const k4_index* ix, uint64_t* prior20);
int k4_load_loci_constraints(k4_index* ix, const char* path, k4_loci_constraint** tbl, int32_t* n, char* errbuf);
/* ---- priority regions (`kalign -B <bed>`, `-V`; kit4b_amd/csrc/k4_priority.hip) ---------------------------------------------------
 * k4_set_priority_regions  <- what CKAligner::Align keeps of its CBEDfile (KAligner.cpp:311-330): n_intervals features as (1-based
 *                             entry id, start, end), 0-based INCLUSIVE loci (a BED line's end column less one), any order; they may
 *                             overlap.  HOST arrays; the index keeps its own device copy until the next call or k4_close.
 *                             n_intervals = 0 clears the table.  Waits for the device.  While a table is set, every
 *                             k4_kalign_*_batch* / k4_kalign_pe_batch* call and a pipeline run CKAligner::ProcCoredApprox's priority
 *                             pass (:9682-9770) in front of the normal call: each read is first aligned for max_ml + 10 hits without
 *                             the microInDel / splice phases; when 1..max_ml of the hits that call reported lie in a feature
 *                             (CBEDfile::InAnyFeature over Seg[0]'s raw MatchLoci .. MatchLoci + MatchLen - 1), the read goes on with
 *                             that many hits -- compacted as :9732-9755 compact them, which is not stable: see k4_priority.hip --
 *                             and with that call's LowMMCnt / NxtLowMMCnt; every other read gets the normal call.  Such a call waits for its stream (the reads that need the normal call are counted on the host),
 *                             and pe_mode 3 / 4 (-X / -N) is turned down with K4_ERR_UNSUPPORTED.  Without a table the calls launch
 *                             what they launched before.
 * k4_filter_priority_regions_dev <- CKAligner::FiltByPriorityRegions (:4093-4155), which kalign runs behind FiltByChroms unless -V was
 *                             given: an accepted read whose Seg[0] span is in no feature of its own sequence becomes
 *                             K4_NAR_REGIONFILT with num_hits = 0 (inst stays) and the ChromID of its hit -- and of its second
 *                             segment, d_seg2, may be NULL -- zeroed.  With no table set no sequence has a feature: every accepted
 *                             read is marked (a BED file that names none of the index's sequences).  pe: d_rr_or_pe holds n_reads
 *                             k4_pe_read records, read by read, else k4_read_result with hit slot 0 of d_hits.  Waits for `stream`.
 * k4_priority_times        <- for tools/priority_bench.py: while k4_enable_kernel_timing is on, the host-clock milliseconds the calls
 *                             spent in the wide pass, the select kernel with the listing, the normal pass with the scatter; and the
 *                             reads that went through the wide pass / that needed the normal pass.  Reading zeroes them. */
enum { K4_NAR_REGIONFILT = 12 /* eNARRegionFilt, KAligner.h:149 */ };
int k4_set_priority_regions(k4_index* ix, int64_t n_intervals, const uint32_t* entry_ids, const uint32_t* starts, const uint32_t* ends);
int k4_filter_priority_regions_dev(k4_index* ix, int pe, int64_t n_reads, int32_t max_ml, void* d_rr_or_pe, void* d_hits, void* d_seg2,
                                   int64_t* n_removed, void* stream);
int k4_priority_times(k4_index* ix, double ms3[3], uint64_t reads2[2]);
/* k4_priority_select_dev   <- the walk of :9724-9763 alone, step (b) of the priority pass, over records the caller supplies: d_wide_rr /
 *                             d_wide_hits hold n_reads results of a call with max_ml + 10 hit slots per read; reads with 1..max_ml
 *                             priority hits get their k4_read_result (classified for pe_mode 0..2) and hits in d_out_rr / d_out_hits
 *                             (max_ml slots per read; the slots behind the instances zeroed unless sparse_hits) and d_need[i] = 0;
 *                             every other read gets d_need[i] = 1 (uint8), its d_out_rr record is left as it was and its hit slots
 *                             are undefined.  Enqueues only.  A feature of no bases is given to k4_set_priority_regions as
 *                             end = start - 1 (start >= 1) and meets a span that covers start - 1 and start, as in the reference. */
int k4_priority_select_dev(k4_index* ix, int64_t n_reads, int32_t max_ml, int32_t pe_mode, int32_t sparse_hits, const void* d_wide_rr,
                           const void* d_wide_hits, void* d_out_rr, void* d_out_hits, void* d_need, void* stream);
int k4_chrom_accept_mask(k4_index* ix, int32_t n_incl, const char* const* incl, int32_t n_excl, const char* const* excl, uint8_t* mask);
/* ---- alignment statistics (`kalign -O <file>`; kit4b_amd/csrc/k4_stats.hip) -------------------------------------------------
 * k4_align_stats_collect <- m_MultiHitDist (KAligner.cpp:9943) and m_pLenDist (:3251, :3408, :3511): on = 1 zeroes two tallies on the
 *                           device which every later k4_kalign_*_batch_dev / k4_kalign_pe_batch_dev call (a pipeline's too) adds
 *                           to: LowHitInstances of the reads AlignRead accepts, and the fragment length of every pair accepted as
 *                           such or through a rescued mate.  on = 0 drops them; off, the align calls do nothing new.
 * k4_align_stats_dev     <- CKAligner::WriteSubDist (:6469-6525) and the counting of ReportTargHitCnts (:5458-5712) over the
 *                           records in HBM as the last global stage left them: n_reads reads (PE: both ends, d_pe; SE: d_rr and
 *                           hit slot 0 of d_hits); max_read_len bounds lens[] and is the row length of the position tables.  The
 *                           quality band of a base is read from bits 4..7 of its read byte, where k4_set_fastq_quality's parse put
 *                           the 4-bit score (all 0, band 0, under -g3).  Fills *out, the run tallies included (zero when they
 *                           were not collected); waits for `stream`.  Release with k4_free_align_stats.
 * k4_write_align_stats   <- the text: WriteBasicCountStats (:4159-4300) into `path` (left empty when no read was accepted),
 *                           ReportTargHitCnts into <path cut at its last '.'>.AlignCntsDist.csv (only when a read was accepted),
 *                           and with pe != 0 <..>.GlobalPEInsertDist.csv (:3092-3146).  n_loaded: the reads behind the length
 *                           filter (RPKM); ml_mode / max_multi: kalign -r / -R (the multihit block is written for -r > 0). */
#define K4_STATS_MULTI 500      /* cMaxMultiHits, KAligner.h:80 */
#define K4_STATS_PE_LEN 100000  /* cPairMaxLen, KAligner.h:88 */
typedef struct {
  uint32_t max_align_len;       /* m_MaxAlignLen: the longest accepted one-segment read */
  uint32_t len_stride;          /* L: row length of q_insts / q_subs (the call's max_read_len) */
  uint32_t n_entries;
  uint32_t reserved;
  uint64_t n_accepted;          /* accepted reads (ReportTargHitCnts counts these, two-segment reads included) */
  uint64_t* q_insts;            /* [4][L] m_AlignQSubDist[band][pos].QInsts */
  uint64_t* q_subs;             /* [4][L] .Subs */
  uint64_t* m_sub;              /* [L + 1] m_AlignMSubDist */
  uint64_t* multi_hit;          /* [K4_STATS_MULTI] m_MultiHitDist */
  uint64_t* pe_len_dist;        /* [K4_STATS_PE_LEN + 1] m_pLenDist */
  uint32_t* ent_hits;           /* [n_entries] accepted alignments per target, by entry order */
  uint32_t* ent_uniq_loci;      /* [n_entries] distinct AdjAlignStartLoci */
  uint32_t* ent_indeterminate;  /* [n_entries] reads whose first three bases hold a non-ACGT */
  uint32_t* ent_trimer;         /* [n_entries][64] reads by their first three bases (A=0 .. T=3, first base most significant) */
  void* block;                  /* the one allocation behind the arrays */
} k4_align_stats;
int k4_align_stats_collect(k4_index* ix, int on);
int k4_align_stats_dev(k4_index* ix, int pe, int64_t n_reads, int32_t max_ml, int32_t max_read_len, const void* d_rr,
                       const void* d_hits, const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens,
                       k4_align_stats* out, void* stream);
void k4_free_align_stats(k4_align_stats* s);
int k4_write_align_stats(k4_index* ix, const k4_align_stats* s, uint64_t n_loaded, int32_t ml_mode, int32_t max_multi, int pe,
                         const char* path);
/* ---- per-target PE insert length distributions (`kalign -3`, --petranslendist; kit4b_amd/csrc/k4_peinserts.hip) ------------------
 * k4_pe_insert_dist_dev    <- the walk of CKAligner::ReportPEInsertLenDist (KAligner.cpp:5321-5454) in the order of SortPEHitMatch
 *                             (:10928-10963) over the pair records in HBM as the last global stage left them (d_pe: 2 x n_pairs
 *                             k4_pe_read, mates at 2q and 2q + 1): the reads that are accepted and FlgPEAligned, by (ChromID, pair,
 *                             PE1 before PE2), taken TWO AT A TIME as the reference takes them -- where a later stage took one mate
 *                             of a pair out, the pairings behind it on that walk shift by one, and a last odd read is dropped.
 *                             With S = AdjAlignStartLoci + 1 and L = AdjAlignHitLen: TLen = S1 <= S2 ? (S2 - S1) + L2 : (S1 - S2) + L1
 *                             in 32-bit unsigned arithmetic, counted on the target of the first of the two: dist[0] TLen < 100,
 *                             dist[51] TLen > 600, else dist[1 + (TLen - 99) / 10].  Only the first 1 000 000 pairs of a target in
 *                             walk order are counted (:5404).  median: CKAligner::MedianInsertLen (:5256-5319), which is not the
 *                             textbook median (k4_pe_insert_median_host is the same rule on the host).  One row per target with a
 *                             pair, ascending entry id.  Changes none of the records; waits for `stream`.  Release with
 *                             k4_free_pe_insert_dist.
 * k4_write_pe_insert_dist  <- the text (:5354-5357, :5383-5386): the header and per row "name",SeqLen,TotPEs,Median,Sum / TotPEs and
 *                             the 52 columns; names and lengths are the index's.  kalign's file is <the -O path>.peinserts.csv
 *                             (:205-215: appended to the whole path).  n_accepted: the accepted reads of the run; the file is
 *                             left empty when it is 0 (:771), else the header is written even without a row.
 * k4_pe_insert_bin_host / k4_pe_insert_median_host: the column of a TLen and MedianInsertLen of `n` values in walk order, on the
 *                             host (no device, no index): the functions the kernels run (values must not hold a 0). */
#define K4_PE_INSERT_BINS 52
typedef struct {
  uint32_t n_rows;
  uint32_t reserved;
  uint32_t* entry_id;   /* [n_rows] 1-based entry id of the target, ascending */
  uint32_t* tot_pes;    /* [n_rows] NumPEs: pairs counted, at most 1 000 000 */
  uint32_t* median;     /* [n_rows] MedianInsertLen over the counted pairs */
  uint64_t* sum;        /* [n_rows] SumInsertLens */
  uint32_t* dist;       /* [n_rows][K4_PE_INSERT_BINS] LenDist */
  void* block;          /* the one allocation behind the arrays */
} k4_pe_insert_dist;
int k4_pe_insert_dist_dev(k4_index* ix, int64_t n_pairs, const void* d_pe, k4_pe_insert_dist* out, void* stream);
void k4_free_pe_insert_dist(k4_pe_insert_dist* d);
int k4_write_pe_insert_dist(k4_index* ix, const k4_pe_insert_dist* d, uint64_t n_accepted, const char* path);
int k4_pe_insert_bin_host(uint32_t tlen);                                                  /* the column, 0..51 */
int k4_pe_insert_median_host(const uint32_t* values, uint32_t n, uint32_t* median);  /* a K4_* code */
/* ---- start-site octamer preferences (`kalign -8 <file>`, `-9 <ofs>`; kit4b_amd/csrc/k4_siteprefs.hip) ---------------------------
 * k4_site_prefs_dev      <- the walk of CKAligner::ProcessSiteProbabilites (KAligner.cpp:8750-8821) over the records in HBM as the last
 *                           global stage left them: n_reads reads (PE: both ends, d_pe; SE: d_rr and hit slot 0 of d_hits).  In
 *                           SortHitMatch order (the order of the SAM body) every accepted one-segment read gives the octamer of the
 *                           target at `ofs` (-100..100, kalign's default -4; else K4_ERR_PARAMS) from its 5' end, located from the raw
 *                           MatchLoci / MatchLen in the reference's 32-bit unsigned arithmetic (a locus in front of the sequence wraps and
 *                           is clamped to the sequence's end, :8778-8782), reverse complemented for a Crick alignment; an octamer that
 *                           holds an N is not counted.  num_occs counts the reads, num_sites the changes of locus along the walk.  A
 *                           read whose signed locus lies in -8..-1 (the reference reads an uninitialised array) is not counted.
 *                           Changes none of the records; waits for `stream`.  Release with k4_free_site_prefs.
 * k4_write_site_prefs    <- the scale step (:8823-8872) and CKAligner::WriteSitePrefs (:8910-8945): per strand NumOccs / NumSites,
 *                           the 64 largest set to 1.000 (a stable sort: ties go to the higher octamers) and every other ratio divided
 *                           by their mean, floor 0.0001; 65535 rows per strand (the reference leaves out tttttttt).  The file is left
 *                           empty when no read was accepted (:743, :780).  Host only; an error's text is in k4_global_error. */
typedef struct {
  uint32_t* num_occs[2];   /* [65536] m_OctSitePrefs[strand][octamer].NumOccs: 0 Watson, 1 Crick; first base most significant */
  uint32_t* num_sites[2];  /* [65536] .NumSites */
  uint64_t n_accepted;     /* accepted reads (two-segment reads included) */
  uint64_t n_counted;      /* reads that were counted */
  void* block;             /* the one allocation behind the arrays */
} k4_site_prefs;
int k4_site_prefs_dev(k4_index* ix, int pe, int64_t n_reads, int32_t max_ml, int32_t ofs, const void* d_rr, const void* d_hits,
                      const void* d_pe, k4_site_prefs* out, void* stream);
void k4_free_site_prefs(k4_site_prefs* s);
int k4_write_site_prefs(const k4_site_prefs* s, const char* path);
/* k4_best_matches_batch <- CSfxArray::LocateBestMatches (SfxArray.h:793, SfxArray.cpp:6836-7205; CKAligner's `-N`) for
 * n_reads reads: at most p->max_hits alignments with no more than p->tot_mm mismatches, sorted by mismatches; rslt = the
 * call's return value (0 none, 1..max_hits, max_hits+1 when further matches were sloughed), inst = alignments in the
 * read's hit slots.  mm_delta and min_core_len of *p are not used; MaxIter is the index's (k4_set_max_iter). */
int k4_best_matches_batch(k4_index* ix, const k4_align_params* p, int64_t n_reads, const uint8_t* reads, const uint64_t* offs,
                          const uint32_t* lens, int32_t* rslt, int32_t* inst, k4_hit* hits);
int k4_best_matches_batch_dev(k4_index* ix, const k4_align_params* p, int64_t n_reads, int32_t max_read_len,
                              const void* d_reads, const void* d_offs, const void* d_lens, void* d_rslt, void* d_inst,
                              void* d_hits, void* stream);

/* ---- blitz: seed and extend ----------------------------------------------------------------------------------
 * k4_locate_query_seqs_batch <- CSfxArray::LocateQuerySeqs (SfxArray.h:779, SfxArray.cpp:6493-6833; CBlitz's engine call) for
 * n_queries sequences of codes 0..4: exact cores of core_len bases every core_delta bases, each occurrence of a core that
 * occurs fewer than max_iter times extended 5' and 3' (match_pts / mismatch_pts, 15 % mismatch cap) unless an earlier node of
 * the same target holds it on its diagonal, overlapping nodes reduced by the reference's redundancy rules, at most max_hits
 * nodes.  strand: 0 both ('+' first), 1 '+', 2 '-' ('-' nodes are in the coordinates of the reverse-complemented query).
 * Output: the nodes of query i are nodes[node_offs[i] .. node_offs[i + 1]), in the reference's order; slot = the reference's
 * AlignNodeID.  When the total exceeds nodes_cap the call returns K4_ERR_MEM, node_offs is complete (node_offs[n_queries] =
 * the capacity needed) and nodes is not written.  max_iter is the call's CurMaxIter, not the index's MaxIter.
 * k4_query_reserve sizes the per-query node slices of the workspace ahead of time (the batch calls grow it when needed; the
 * index owns it, k4_close frees it).  k4_query_last_kernel_ms: device time of the last batch's kernels. */
typedef struct {
  int32_t core_len;     /* 8..100 */
  int32_t core_delta;   /* >= 1 */
  int32_t strand;
  int32_t max_hits;     /* >= 1 */
  int32_t max_iter;
  int32_t match_pts;
  int32_t mismatch_pts;
} k4_query_params;
typedef struct {
  uint32_t query_start;
  uint32_t align_len;
  uint32_t targ_seq_id;
  uint32_t targ_loci;
  uint32_t n_mismatches;
  uint32_t slot;
  uint32_t strand;      /* 0 '+', 1 '-' */
} k4_query_node;
int k4_query_reserve(k4_index* ix, const k4_query_params* p, int64_t max_queries, uint32_t max_query_len);
int k4_locate_query_seqs_batch(k4_index* ix, const k4_query_params* p, int64_t n_queries, const uint8_t* seqs, const uint64_t* offs,
                               const uint32_t* lens, uint64_t* node_offs, k4_query_node* nodes, uint64_t nodes_cap);
int k4_locate_query_seqs_batch_dev(k4_index* ix, const k4_query_params* p, int64_t n_queries, uint32_t max_query_len,
                                   const void* d_seqs, const void* d_offs, const void* d_lens, void* d_node_offs, void* d_nodes,
                                   uint64_t nodes_cap, void* stream);
double k4_query_last_kernel_ms(const k4_index* ix);

/* ---- blitz: the path stage -----------------------------------------------------------------------------------
 * k4_blitz_paths_batch <- what CBlitz (libkit4b/CBlitz.cpp) does with the nodes of a query before it writes a line: the nodes
 * sorted (SortQueryAlignNodes), chained into scored paths per target and strand (IdentifyHighScorePaths, HighScoreSW), the best
 * max_paths heads of the query kept, each path consolidated base by base against the target (ConsolidateNodes), characterised
 * (CharacterisePath) and counted (BlocksAlignStats).  Input: the queries and the node_offs / nodes k4_locate_query_seqs_batch[_dev]
 * produced for them (match_pts / mismatch_pts as in that call).  Nodes a caller made itself must lie inside their query and
 * target; a query under 8 bases, which is shorter than any node, gets no path.  Output: the paths of query i are paths[path_offs[i] ..
 * path_offs[i + 1]) in the reference's report order, the blocks of a path blocks[block_off .. block_off + n_blocks).  q_start ..
 * t_end are inclusive and, on strand 1, in the coordinates of the reverse-complemented query, as CBlitz::Report passes them on.
 * needed[0] / needed[1] (host, always written): the paths and blocks found.  When either exceeds its capacity the call returns
 * K4_ERR_MEM and writes nothing to path_offs, paths and blocks.  Parameters outside their ranges give K4_ERR_PARAMS.
 * The _dev form takes device pointers (needed stays a host pointer) and a stream, and returns when the stream has finished.
 * The index owns the workspace.  k4_blitz_last_kernel_ms: device time of the last batch. */
typedef struct {
  int32_t match_pts;              /* 1..10 */
  int32_t mismatch_pts;           /* 1..10 */
  int32_t gap_open;               /* 1..50 */
  int32_t min_path_score;         /* 0 = ((query length - 5) * match_pts) / 3; floored at 25 */
  int32_t query_len_aligned_pct;  /* 1..100 */
  int32_t max_paths;              /* 1..10 */
  int32_t strand;                 /* 0 both, 1 '+', 2 '-' */
} k4_blitz_params;
typedef struct {
  uint32_t query;        /* index in the batch */
  uint32_t targ_seq_id;
  uint32_t strand;       /* 0 '+', 1 '-' */
  uint32_t score;
  uint32_t matches, mismatches, n_count;
  uint32_t q_num_insert, q_base_insert, t_num_insert, t_base_insert;
  uint32_t q_start, q_end, t_start, t_end;
  uint32_t n_blocks;
  uint64_t block_off;
} k4_blitz_path;
typedef struct {
  uint32_t len, q_start, t_start;
} k4_blitz_block;
int k4_blitz_paths_batch(k4_index* ix, const k4_blitz_params* p, int64_t n_queries, const uint8_t* seqs, const uint64_t* offs,
                         const uint32_t* lens, const uint64_t* node_offs, const k4_query_node* nodes, uint64_t* path_offs,
                         k4_blitz_path* paths, uint64_t paths_cap, k4_blitz_block* blocks, uint64_t blocks_cap, uint64_t* needed);
int k4_blitz_paths_batch_dev(k4_index* ix, const k4_blitz_params* p, int64_t n_queries, const void* d_seqs, const void* d_offs,
                             const void* d_lens, const void* d_node_offs, const void* d_nodes, void* d_path_offs, void* d_paths,
                             uint64_t paths_cap, void* d_blocks, uint64_t blocks_cap, uint64_t* needed, void* stream);
double k4_blitz_last_kernel_ms(const k4_index* ix);

/* ---- restricted Hammings ---------------------------------------------------------------------------------------
 * k4_locate_sfx_hammings_batch <- CSfxArray::LocateSfxHammings (SfxArray.cpp:4107-4220) and k4_locate_hammings_batch <-
 * CSfxArray::LocateHammings (:4227-4331), both over LocateHamming (:4339-4627; `ngskit4b hammings -m0`): for every sample_nth-th
 * K-mer of a span the number of substitutions to the nearest other K-mer of the index, found by the reference's escalation
 * (0,1) -> (2,2) -> (3,3) -> (4,4) -> (5,rhamm) with its core depths, so it misses what the reference misses.  One call takes
 * n_spans spans, each what one call of the reference takes:
 *   sfx form   span i = span_lens[i] bases of entry entry_ids[i] from locus entry_locis[i]; the K-mers know their own place
 *   seq form   span i = lens[i] codes (etSeqBase) at seqs + offs[i]; ProbeEntry 0: no self hit, no intra / inter filter
 * and writes hammings[out_offs[i] + j] for j = 0, nth, 2 nth .. <= span length - kmer_len: every other byte of hammings stays
 * as it was (the reference's callers fill it with 0xFF).  The sfx form clamps a byte at 20 as the reference does.
 * Errors, nothing written: rhamm < 1, kmer_len outside 10..500, a null array, entry id 0 or unknown, a span that leaves its
 * entry or is shorter than kmer_len give K4_ERR_INTERNAL (the reference's eBSFerrInternal); narrower than the reference, rhamm
 * > 10, kmer_len / (rhamm + 1) < 8, intra_inter_both outside 0..2 or a span whose bytes leave hammings_len give K4_ERR_PARAMS.
 * The span arrays are host memory in both forms; the _dev forms take hammings (and seqs) as device pointers and a stream and
 * return when the stream has finished.  A batch goes out in launches of a fixed number of K-mers.  The index owns the
 * workspace.  k4_hamming_last_kernel_ms: device time of the last batch's launches. */
typedef struct {
  int32_t rhamm;             /* 1..10 */
  int32_t kmer_len;          /* 10..500, kmer_len / (rhamm + 1) >= 8 */
  int32_t sample_nth;        /* <= 0: 1 */
  int32_t both_strands;      /* bSAHammings */
  uint32_t min_core_depth;
  uint32_t max_core_depth;
  int32_t intra_inter_both;  /* 0 both, 1 intra only, 2 inter only */
} k4_hamming_params;
int k4_locate_sfx_hammings_batch(k4_index* ix, const k4_hamming_params* p, int64_t n_spans, const uint32_t* entry_ids,
                                 const uint32_t* entry_locis, const uint32_t* span_lens, const uint64_t* out_offs, uint8_t* hammings,
                                 uint64_t hammings_len);
int k4_locate_sfx_hammings_batch_dev(k4_index* ix, const k4_hamming_params* p, int64_t n_spans, const uint32_t* entry_ids,
                                     const uint32_t* entry_locis, const uint32_t* span_lens, const uint64_t* out_offs, void* d_hammings,
                                     uint64_t hammings_len, void* stream);
int k4_locate_hammings_batch(k4_index* ix, const k4_hamming_params* p, int64_t n_spans, const uint8_t* seqs, const uint64_t* offs,
                             const uint32_t* lens, const uint64_t* out_offs, uint8_t* hammings, uint64_t hammings_len);
int k4_locate_hammings_batch_dev(k4_index* ix, const k4_hamming_params* p, int64_t n_spans, const void* d_seqs, const uint64_t* offs,
                                 const uint32_t* lens, const uint64_t* out_offs, void* d_hammings, uint64_t hammings_len, void* stream);
double k4_hamming_last_kernel_ms(const k4_index* ix);

/* ---- K-mer cultivar counts -------------------------------------------------------------------------------------
 * k4_kmer_cults_batch <- CSfxArray::GenKMerCultsCnts with AntisenseKMerCultsCnts (SfxArray.cpp:2804-3133; `ngskit4b kmermarkers`),
 * MaxHomozygotic 0: over the suffix array elements start_sfx_idx .. end_sfx_idx (inclusive; 0 or beyond the array: to its end)
 * every run of suffixes that share an ACGT-only prefix of prefix_len bases and are followed by suffix_len more ACGT bases is one
 * located K-mer; per entry ("cultivar") its sense occurrences inside the range and, unless sense_only, the occurrences of the
 * prefix's reverse complement in the whole index.  A K-mer found in min_cultivars entries or more (0: all) is reported, in
 * suffix order:
 *   kmers[i]  the suffix index of its first element, its totals (saturating at 2^32 - 1), how many entries hold it, and where
 *             its counts start in dist
 *   bases     prefix_len + suffix_len codes per K-mer
 *   dist      {entry_id, sense, antisense} of the entries with a count, by ascending place in the entry table
 * The call is resumable: it writes whole K-mers while caps hold them and returns in totals how many K-mers it located
 * (reported or not), how many records it wrote, and next_sfx_idx, the first element it did not process -- always the start of a
 * run, so a call that starts there continues with the records one big call would have written next; done != 0: the range is
 * finished.  The range goes through in windows of at most max_window elements (0: 2^20; capped at 2^24), whatever the length
 * of a run, and the workspace, which the index owns, is sized by the window and the number of entries alone.
 * A window holds no more elements than the outputs have room left (floor 4096), so little room means little work per call; one
 * call writes at most 2^21 K-mers and 2^25 counts whatever the caps say, and the host-pointer form stages that much on the device.
 * Errors, nothing written: the reference's own (prefix_len outside 5..200, suffix_len outside 0..200, their sum above 300,
 * min_cultivars below 0 or above the number of entries, more than 20000 entries, a negative index, start_sfx_idx beyond the
 * array) give K4_ERR_INTERNAL, the reference's -1; max_homozygotic > 0 with a suffix (the homozygotic check depends on the
 * order of the sequential walk) gives K4_ERR_UNSUPPORTED, and without a suffix it is ignored as the reference ignores it; a
 * null argument, max_window < 0, max_kmers < 1 or max_dist below the number of entries give K4_ERR_PARAMS.
 * The _dev form takes device pointers in its k4_cults_out and a stream and returns when the stream has finished.
 * k4_cults_last_kernel_ms: device time of the last call's launches.  k4_get_sfx_els: n suffix array elements from `first`
 * (SfxOfsToLoci), for GenKMerCultThreadRange on the host. */
typedef struct {
  int32_t prefix_len;       /* 5..200 */
  int32_t suffix_len;       /* 0..200, prefix_len + suffix_len <= 300 */
  int32_t min_cultivars;    /* 0: all entries */
  int32_t sense_only;
  int32_t max_window;       /* 0: the default */
  int32_t max_homozygotic;  /* 0, or anything without a suffix */
} k4_cults_params;
typedef struct {
  uint64_t head_sfx_idx;
  uint64_t dist_ofs;
  uint32_t sense_cnts, antisense_cnts, num_cultivars, reserved;
} k4_cult_kmer;
typedef struct { uint32_t entry_id, sense, antisense; } k4_cult_dist;
typedef struct { k4_cult_kmer* kmers; uint8_t* bases; k4_cult_dist* dist; } k4_cults_out;
typedef struct { uint64_t max_kmers, max_dist; } k4_cults_caps;
typedef struct { int64_t n_located; uint64_t n_kmers, n_dist, next_sfx_idx; int32_t done, reserved; } k4_cults_totals;
int k4_kmer_cults_batch(k4_index* ix, const k4_cults_params* p, int64_t start_sfx_idx, int64_t end_sfx_idx, const k4_cults_out* out,
                        const k4_cults_caps* caps, k4_cults_totals* totals);
int k4_kmer_cults_batch_dev(k4_index* ix, const k4_cults_params* p, int64_t start_sfx_idx, int64_t end_sfx_idx, const k4_cults_out* d_out,
                            const k4_cults_caps* caps, k4_cults_totals* totals, void* stream);
double k4_cults_last_kernel_ms(const k4_index* ix);
int k4_get_sfx_els(k4_index* ix, uint64_t first, uint64_t n, uint64_t* els);

/* ---- kmarkers: exact ranges and the species scan -----------------------------------------------------------------
 * k4_exact_ranges_batch <- CSfxArray::IterateExacts walked to its end (SfxArray.cpp:3381-3458): for probe i (lens[i] codes at
 * seqs + offs[i], compared on the low nibble as CmpProbeTarg does, never across an end-of-sequence symbol) firsts[i] = the suffix
 * index of its first exact match and counts[i] = how many suffixes match (saturating at 2^32 - 1); 0 and 0 without a match or for
 * an empty probe.  firsts[i] + 1 is what IterateExacts(probe, len, 0, ..) returns, and the hits it then iterates are the
 * elements firsts[i] .. firsts[i] + counts[i] - 1.  The _dev form takes every array as a device pointer.
 * k4_matches_other_chroms_batch <- CSfxArray::MatchesOtherChroms (:5094-5235), probe i against the entries whose ids are not among
 * ids[0 .. n_ids): matches[i] = 1 or 0, as the reference returns it -- a hit of a core (CoreLen = max(8, len / (1 + max_tot_mm)),
 * offsets 0, CoreLen, .. below len - CoreLen) on another entry over which the probe can be laid returns 1 whatever the flanks
 * hold.  n_ids 0..50, probes of at most 500 bases, else K4_ERR_PARAMS.  Host pointers.
 * k4_species_kmers_batch <- CLocKMers::LocateSpeciesUniqueKMers (ngskit4b/LocKMers.cpp:1085-1232; `ngskit4b kmarkers`) as ONE thread
 * runs it: status[pre(t) + l] for start locus l of target t, the targets in the order of target_ids (the front end's: sorted by
 * name without case), pre(t) = the summed lengths of the targets in front.  A status is the first of
 *   1  fewer than kmer_len ACGT bases from here to the next other symbol or the entry's end
 *   2  the K-mer's first exact hit is in an entry that is no target
 *   3  duplicate: the K-mer or, where the reverse complement's first hit is in a target, its reverse complement stands at an
 *      earlier (target, locus); a K-mer that is its own reverse complement is one wherever it stands
 *   4  a hit of the K-mer, or a hit of its reverse complement other than that strand's first, is in an entry that is no target
 *   5  min_hamming > 1 and MatchesOtherChroms(targets, min_hamming - 1, K-mer) or (.., reverse complement) is 1
 *   6  mode 2: fewer than min_with_prefix (0, or more than there are: all) entries that are no targets hold the first prefix_len
 *      bases of the K-mer or of its reverse complement
 *   7  accepted
 * totals: processed (status > 1), cultivar_specific (> 4), hamming_retained (> 5), accepted = the markers the front end writes:
 * the accepted K-mers in modes 0 and 2, in mode 1 the runs of adjacent accepted K-mers that a later accepted K-mer of the same ACGT
 * run follows (the front end never flushes the last).  Nothing is written into the index.  status_len >= the summed lengths of
 * the targets; the bytes behind them are not touched.  K4_ERR_PARAMS: kmer_len outside 20..100, min_hamming outside 1..5, mode
 * outside 0..2, in mode 2 prefix_len outside 10..kmer_len - 10, an unknown or repeated target id, more than 50 targets, targets
 * that are all the entries, a null argument, status_len too small.  K4_ERR_UNSUPPORTED: an ACGT run of 0x7fffe bases or more in
 * a target (the front end stops handing out blocks there), mode 2 over more than 2048 entries.  The _dev form takes status as a
 * device pointer and a stream and returns when the stream has finished.  k4_kmarkers_last_kernel_ms: device time of the last of
 * these calls' launches. */
typedef struct {
  int32_t kmer_len;         /* 20..100 */
  int32_t min_hamming;      /* 1..5 */
  int32_t mode;             /* 0 | 1 | 2 */
  int32_t prefix_len;       /* mode 2: 10..kmer_len - 10 */
  int32_t min_with_prefix;  /* mode 2; 0: every entry that is no target */
  int32_t reserved;
} k4_kmarkers_params;
typedef struct { uint64_t processed, cultivar_specific, hamming_retained, accepted; } k4_kmarkers_totals;
int k4_exact_ranges_batch(k4_index* ix, int64_t n, const uint8_t* seqs, const uint64_t* offs, const uint32_t* lens, uint64_t* firsts,
                          uint32_t* counts);
int k4_exact_ranges_batch_dev(k4_index* ix, int64_t n, const void* d_seqs, const void* d_offs, const void* d_lens, void* d_firsts,
                              void* d_counts, void* stream);
int k4_matches_other_chroms_batch(k4_index* ix, int32_t n_ids, const uint32_t* ids, int32_t max_tot_mm, int64_t n, const uint8_t* seqs,
                                  const uint64_t* offs, const uint32_t* lens, int32_t* matches);
int k4_species_kmers_batch(k4_index* ix, const k4_kmarkers_params* p, int32_t n_targets, const uint32_t* target_ids, uint8_t* status,
                           uint64_t status_len, k4_kmarkers_totals* totals);
int k4_species_kmers_batch_dev(k4_index* ix, const k4_kmarkers_params* p, int32_t n_targets, const uint32_t* target_ids, void* d_status,
                               uint64_t status_len, k4_kmarkers_totals* totals, void* stream);
double k4_kmarkers_last_kernel_ms(const k4_index* ix);

/* ---- genzygosity: LocateAllNearMatches and the scan ----------------------------------------------------------------
 * k4_all_near_matches_batch <- CSfxArray::LocateAllNearMatches (SfxArray.cpp:4820-5091): probe i (lens[i] codes at seqs + offs[i],
 * compared on the low nibble) came from entry id probe_entries[i] at probe_ofs[i].  Both strands; cores of core_len at 0, then
 * every core_delta, the last one right-aligned (:4906-4917), at most max_core_slides per strand; a candidate is extended over the
 * whole probe with at most max_tot_mm mismatches and never across an end-of-sequence symbol.  rslts[i] = -1 when a match lies in
 * the probe's own entry at another locus, or when a match in another entry arrives after max_matches (> 0) of them; else the
 * number of matches in other entries.  counts (may be null): counts[i * n_entries + id - 1] = matches in the entry with that id
 * (ids above n_entries are not counted), on a -1 as the reference's walk had them when it returned.  cur_max_iter (0: none) and
 * n_ident_nodes limit the walk as CurMaxIter and NumAllocdIdentNodes do, the check at the 100th iteration included.
 * K4_ERR_PARAMS: a probe over 1000 bases or shorter than core_len, core_len or core_delta below 1, max_core_slides outside
 * 1..32, a limit below 0, a null argument, counts_cap < n * n_entries with counts given.
 * k4_zygosity_batch <- genzygosity (genzygosity/genzygosity.cpp:1122-1236, the derivation of :681-697 and :998-1027): every
 * subseq_len window of the source entries src_first .. src_first + src_count - 1 (ordinals 1..n_entries of the entry table) is
 * passed over when it holds a code above N or more than max_ns N, else asked with CoreLen = max(MinCoreLen, subseq_len /
 * (max_subs + 1)), MaxIter and the slides of `mode`, and 1 024 000 ident nodes.  matrix[r * n_entries + id - 1] = the windows of
 * source r unique to it that matched the entry with that id, subseqs[r] = its unique windows.  status (may be null), one byte per
 * start locus of the source entries in order: 0 passed over (or no window starts here), 1 the call returned -1, 2 unique
 * without a match elsewhere, 3 unique with.  An entry shorter than subseq_len has no windows (the reference's front end never
 * gets past such an entry); no window fits into it either, so its row and its column stay 0.  totals.ordered: the windows that
 * needed the sequential walk; second_launch: those among them whose dedupe set went to device memory.  K4_ERR_PARAMS: subseq_len outside 20..1000, max_subs outside
 * 0..min(30, subseq_len - 18), max_ns outside 0..5, max_matches outside 0..1000000, mode outside 0..3, source entries outside
 * 1..n_entries, status_len below the source entries' loci, a null argument.  K4_ERR_UNSUPPORTED: more than 16384 entries.
 * Nothing is written into the index.  The _dev forms take every array as a device pointer and a stream, and return when the
 * stream has finished.  k4_zygosity_last_kernel_ms: the time on the stream from the first launch of the last of these calls to
 * its last, 0 when it launched none.  Between them the host looks at the list of deferred probes, once in a given-probe call and
 * once per 64 launches (1 048 576 start loci) of the scan: that wait is in the figure. */
typedef struct {
  int32_t max_tot_mm, core_len, core_delta, max_core_slides;
  int32_t max_matches;    /* 0: no limit */
  int32_t cur_max_iter;   /* 0: no limit */
  int32_t n_ident_nodes;  /* NumAllocdIdentNodes */
  int32_t reserved;
} k4_near_params;
typedef struct {
  int32_t subseq_len;   /* -l 20..1000 */
  int32_t max_subs;     /* -s */
  int32_t max_ns;       /* -n 0..5 */
  int32_t max_matches;  /* -x 0..1000000, 0: no limit */
  int32_t mode;         /* -m 0..3 */
  int32_t reserved;
} k4_zygosity_params;
typedef struct { uint64_t windows, passed_over, rejected, unique, unique_matched, ordered, second_launch; } k4_zygosity_totals;
int k4_all_near_matches_batch(k4_index* ix, const k4_near_params* p, int64_t n, const uint8_t* seqs, const uint64_t* offs, const uint32_t* lens,
                              const uint32_t* probe_entries, const uint32_t* probe_ofs, int32_t* rslts, uint32_t* counts, uint64_t counts_cap);
int k4_all_near_matches_batch_dev(k4_index* ix, const k4_near_params* p, int64_t n, const void* d_seqs, const void* d_offs, const void* d_lens,
                                  const void* d_probe_entries, const void* d_probe_ofs, void* d_rslts, void* d_counts, uint64_t counts_cap,
                                  void* stream);
int k4_zygosity_batch(k4_index* ix, const k4_zygosity_params* p, int32_t src_first, int32_t src_count, uint32_t* matrix, uint32_t* subseqs,
                      uint8_t* status, uint64_t status_len, k4_zygosity_totals* totals);
int k4_zygosity_batch_dev(k4_index* ix, const k4_zygosity_params* p, int32_t src_first, int32_t src_count, void* d_matrix, void* d_subseqs,
                          void* d_status, uint64_t status_len, k4_zygosity_totals* totals, void* stream);
double k4_zygosity_last_kernel_ms(const k4_index* ix);

/* ---- paired ends -----------------------------------------------------------------------------------------
 * k4_mate_rescue_batch <- CSfxArray::AlignPairedRead (SfxArray.h:880, SfxArray.cpp:8571-8767; MinChimericLen 0, insert
 *                         window < 1000 => the linear-scan branch :8731-8766 with AdaptiveTrim's full-length rule :5612-5638)
 * k4_kalign_pe_batch   <- the PE flow of CKAligner: ProcCoredApprox (KAligner.cpp:10160-10239: both ends aligned as SE
 *                         with MaxHits 10, multi x multi resolution) + ProcessPairedEnds (:3159-3596: AcceptProvPE,
 *                         PEInsertSize, orphan rescue, NAR reassignment).  out[2i] = PE1 of pair i, out[2i+1] = PE2. */
enum { K4_NAR_CHROMFILT = 11, K4_NAR_PEINSERTMIN = 13, K4_NAR_PEINSERTMAX = 14, K4_NAR_PENOHIT = 15, K4_NAR_PESTRAND = 16,
       K4_NAR_PECHROM = 17, K4_NAR_PEUNALIGN = 18,
       K4_NAR_LOCICONSTRAINED = 19 /* eNARLociConstrained: a base of the read violates a loci base constraint (k4_filter_loci_constraints_dev) */ };  /* eNAR, KAligner.h:136-158 */
typedef struct {
  int32_t pe_mode;      /* etPEproc (KAligner.h:278-282): 1 orphan recovery, 2 unique only, 3 orphanSE, 4 uniqueSE */
  int32_t pair_min_len; /* -d */
  int32_t pair_max_len; /* -D */
  int32_t pair_strand;  /* -E */
} k4_pe_params;
typedef struct {        /* the tsReadHit fields that matter after ProcessPairedEnds */
  int32_t nar;
  int32_t num_hits;
  int32_t inst;
  int32_t low_mm;
  int32_t pe_aligned;   /* FlgPEAligned */
  int32_t rescued;      /* 1 when the hit came from the mate rescue */
  k4_hit hit;
} k4_pe_read;
typedef struct {        /* one AlignPairedRead call */
  uint32_t chrom_id;    /* ChromID of the anchored mate */
  uint32_t start_loci;  /* StartLoci / EndLoci of the anchored mate */
  uint32_t end_loci;
  uint32_t read_len;    /* ReadLen of the mate to place */
  uint64_t read_off;    /* its bases: reads[read_off .. read_off+read_len) (etSeqBase bytes, sense as sequenced) */
  int32_t b3prime_extend;
  int32_t antisense;
  int32_t min_insert;
  int32_t max_insert;
  int32_t max_allowed_mm;
  uint32_t chimeric;    /* 0, or MinChimericLen (15..99) | CoreLen << 8 | CoreDelta << 20: AlignPairedRead's chimeric mode */
} k4_rescue_task;
int k4_mate_rescue_batch(k4_index* ix, int64_t n_tasks, const k4_rescue_task* tasks, const uint8_t* reads,
                         uint64_t reads_bytes, int32_t* rslt, k4_hit* hits);
int k4_kalign_pe_batch(k4_index* ix, const k4_kalign_params* p, const k4_pe_params* pe, int64_t n_pairs,
                       const uint8_t* reads1, const uint64_t* offs1, const uint32_t* lens1, const uint8_t* reads2,
                       const uint64_t* offs2, const uint32_t* lens2, k4_pe_read* out);
/* Device-resident form: reads interleaved (read 2i = PE1 of pair i, read 2i+1 = its PE2), every array in HBM; the SE
 * pass, the pairing kernel (AcceptProvPE / PEInsertSize / NAR reassignment, one thread per pair) and the orphan kernel
 * (AlignPairedRead, one wave per orphan pair) are enqueued on `stream`, which is then waited for. */
int k4_kalign_pe_batch_dev(k4_index* ix, const k4_kalign_params* p, const k4_pe_params* pe, int64_t n_pairs,
                           int32_t max_read_len, const void* d_reads, const void* d_offs, const void* d_lens,
                           void* d_out, void* stream);

/* ---- read ingest and SAM emit on the device ----------------------------------------------
 * k4_parse_fastx_dev   <- CKAligner::LoadRawReads (KAligner.cpp:11648-12421) over CFasta: FASTA ('>', sequence over any
 *                         number of lines) or FASTQ ('@', four lines per record) text resident in HBM -> etSeqBase reads
 *                         (a/c/g/t/u either case -> 0..3, '-' -> 6, other letters -> 4, anything else sloughed:
 *                         CFasta::ReadSequence / Ascii2Sense, Fasta.cpp:1172,1657), offsets, lengths, and the span of
 *                         each descriptor up to its first white space (<= 79 bytes; FASTA: behind leading blanks).  A chunk that is not the last one may end inside a
 *                         record: info->consumed tells how many bytes were used; resubmit the rest in front of the next
 *                         chunk.  The bases go to d_reads[reads_base ...) (room for text_bytes + 16 bytes), offs are
 *                         relative to d_reads; name offsets are text_base + offset in this chunk; the per-record arrays
 *                         hold max_records elements.
 * k4_prepare_reads_dev <- the length filter of LoadRawReads (:12024-12060; a pair is dropped when either mate fails) and
 *                         the PE1/PE2 interleave: slots of dropped reads stay in place with length 0.
 * k4_format_sam_dev    <- WriteBAMReadHits (:5718-5914) / ReportBAMread (:5957-6320) / SortHitMatch (:10969) /
 *                         CSAMfile::AddAlignment (SAMfile.cpp:2194-2377): the accepted reads as SAM lines in coordinate
 *                         order (chrom, start, len, strand, mismatches, then load order), in a buffer this call
 *                         allocates (*d_sam, release with k4_free_device); header lines are the caller's.  SE with
 *                         max_ml > 1 (eMLall): a read contributes one line per reported instance (NumHits).  Also the
 *                         ReportAlignStats tallies and which chromosomes received a hit (for the @SQ rule of :5785-5821). */
enum { K4_FASTA = 1, K4_FASTQ = 2 };
typedef struct {
  uint64_t n_records;
  uint64_t consumed;     /* text bytes that belonged to the records returned */
  uint64_t n_bases;
  uint32_t max_len;
  uint32_t format;       /* K4_FASTA | K4_FASTQ */
} k4_parse_info;
typedef struct {          /* where the QNAMEs live: [0] the reads / PE1 file, [1] the PE2 file (PE only) */
  const void* d_text[2];
  const void* d_name_off[2]; /* uint64 per record: byte offset into d_text */
  const void* d_name_len[2]; /* uint32 per record */
} k4_sam_names;
typedef struct {
  uint64_t nar[20];      /* reads per eNAR value (slots of dropped reads are not counted) */
  uint64_t plus, minus;  /* accepted alignments per strand */
  uint64_t n_lines;      /* SAM lines written */
} k4_sam_stats;
int k4_parse_fastx_dev(k4_index* ix, const void* d_text, uint64_t text_bytes, uint64_t text_base, int final_chunk,
                       int format /* 0: from the first byte */, int64_t max_records, void* d_reads, uint64_t reads_base,
                       void* d_offs, void* d_lens, void* d_name_off, void* d_name_len, k4_parse_info* info, void* stream);
int k4_prepare_reads_dev(k4_index* ix, int pe, int64_t n_units, int32_t min_len, int32_t max_len, const void* d_offs1,
                         const void* d_lens1, const void* d_offs2, const void* d_lens2, uint64_t reads2_base,
                         void* d_offs_out, void* d_lens_out, uint64_t* n_under, uint64_t* n_over, uint32_t* max_read_len,
                         void* stream);
/* ... with kalign's end trims (`-y` / `-Y`: KAligner.cpp:12254-12260, the length tests over the trimmed lengths :12040-12090) and
 * its sampling (`-#<n>`, :11983-11989: of the file's reads / pairs every n-th is loaded, the first included; first_unit = index in
 * the file of this call's first unit; 0 / 1: all) */
int k4_prepare_reads_trim_dev(k4_index* ix, int pe, int64_t n_units, int32_t min_len, int32_t max_len, int32_t trim5, int32_t trim3,
                              int32_t sample_nth, int64_t first_unit, const void* d_offs1, const void* d_lens1, const void* d_offs2, const void* d_lens2, uint64_t reads2_base,
                              void* d_offs_out, void* d_lens_out, uint64_t* n_under, uint64_t* n_over, uint32_t* max_read_len,
                              void* stream);
/* ---- contaminant flank trimming (`kalign -H <file>`, --contaminants; kit4b_amd/csrc/k4_contam.hip) --------------------------
 * k4_load_contaminants   <- CContaminants::LoadContaminantsFile (libkit4b/Contaminants.cpp:211-443) with AddFlankContam (:650-816) and
 *                           FinaliseContaminants (:449): a multi-FASTA, plain or gzip, of 4..200 bases A, C, G, T or N per record.  The
 *                           first word of the descriptor is the name; `@` and digits behind it name the classes (1 5' of SE/PE1, 2 5' of
 *                           PE2, 3 3' of SE/PE1, 4 3' of PE2, 5..8 the same for the reverse complement); without a code, or without a
 *                           descriptor, classes 1, 2, 5 and 6.  One k4_contaminant per (record, class), at most 1600; *tbl is malloc'd
 *                           (k4_free_host), ordered by class and falling length.  What the reference refuses (a length outside 4..200, an
 *                           illegal base, a name or a sequence twice in one class, too many entries, nothing loaded) gives K4_ERR_PARSE /
 *                           K4_ERR_PARAMS with the reference's sentence in k4_last_error (ix may be NULL) and, when errbuf is not NULL, in
 *                           errbuf (256 bytes).  A `&` (vector, containment) record gives K4_ERR_UNSUPPORTED.  Host only.
 * k4_contam_match_host   <- CContaminants::MatchContaminants (:1243-1325) as the plain rule its trie answers (k4_contam_rule.h): the
 *                           largest overlap L >= max(min_overlap, 1) of a contaminant of class cls (0..3) onto the read end, 0 for none,
 *                           for a read outside 20..2000 bases or a class without entries.  read_bases: etSeqBase bytes (bits 0..2 count).
 *                           < 0: a K4_* code.  Host only: no device, no index.
 * k4_contam_trims_dev    <- the calls of LoadRawReads (ngskit4b/KAligner.cpp:11992-12039) for every read of a parsed chunk, as
 *                           k4_parse_fastx_dev left it (PE: both ends, d_offs2 / d_lens2, their offsets relative to d_reads +
 *                           reads2_base): d_contam5[r] / d_contam3[r] (bytes; PE: r = 2i for PE1 and 2i + 1 for PE2 of pair i) = the overlap
 *                           beyond the end trim, max(L - trim5, 0) / max(L - trim3, 0) with a minimum overlap of trim + 1.  Units that
 *                           `-#` (sample_nth, first_unit as in k4_prepare_reads_trim_dev) does not load get 0.  totals4 (host, may be NULL):
 *                           reads with a 5' / 3' trim among PE1, then among PE2, before any length test.  tbl: HOST array.  Waits for
 *                           `stream`.
 * k4_prepare_reads_contam_dev: k4_prepare_reads_trim_dev with the per-read trims beside trim5 / trim3 (either array NULL: zeros): the length
 *                           tests go over trim5 + trim3 + contam5 + contam3 (:12041-12075), a kept read starts trim5 + contam5 bases in and
 *                           loses trim3 + contam3 at its end (:12254-12261, :12280-12286; the quality of a base lives in its byte and goes
 *                           with it).  n_contam4 (host, may be NULL): the reference's four totals (:12262-12265, :12287-12290), the KEPT
 *                           reads with a 5' / 3' contaminant trim among PE1, then among PE2. */
typedef struct {
  uint8_t cls;          /* teContamType: 0 5' of SE/PE1, 1 5' of PE2, 2 3' of SE/PE1, 3 3' of PE2 */
  uint8_t len;          /* 4..200 */
  uint8_t revcpl;       /* the record's reverse complement (codes 5..8) */
  uint8_t reserved[5];
  /* one bit per base in 256 positions: the two bits of A=0 C=1 G=2 T=3, and "is N".  5' classes: base k of len at position
   * 256 - len + k (the suffix ends at 255); 3' classes: base k at position k */
  uint64_t p0[4], p1[4], nmask[4];
} k4_contaminant;
int k4_load_contaminants(k4_index* ix, const char* path, k4_contaminant** tbl, int32_t* n, char* errbuf);
int k4_contam_match_host(const k4_contaminant* tbl, int32_t n, int32_t cls, int32_t min_overlap, const uint8_t* read_bases,
                         int32_t read_len);
int k4_contam_trims_dev(k4_index* ix, const k4_contaminant* tbl, int32_t n, int pe, int64_t n_units, int32_t trim5, int32_t trim3,
                        int32_t sample_nth, int64_t first_unit, const void* d_reads, const void* d_offs1, const void* d_lens1,
                        const void* d_offs2, const void* d_lens2, uint64_t reads2_base, void* d_contam5, void* d_contam3,
                        uint64_t* totals4, void* stream);
int k4_prepare_reads_contam_dev(k4_index* ix, int pe, int64_t n_units, int32_t min_len, int32_t max_len, int32_t trim5, int32_t trim3,
                                int32_t sample_nth, int64_t first_unit, const void* d_offs1, const void* d_lens1, const void* d_offs2,
                                const void* d_lens2, uint64_t reads2_base, const void* d_contam5, const void* d_contam3,
                                void* d_offs_out, void* d_lens_out, uint64_t* n_under, uint64_t* n_over, uint32_t* max_read_len,
                                uint64_t* n_contam4, void* stream);
int k4_format_sam_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                      const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens,
                      const k4_sam_names* names, void** d_sam, uint64_t* sam_bytes, k4_sam_stats* stats,
                      uint8_t* chrom_hit /* host, n_entries + 1 bytes, or NULL */, void* stream);
/* the same with the second segments (d_seg2: one k4_seg2 per read, or NULL): CIGAR with soft clips for trimmed hits and
 * I / D / N between the segments, MAPQ scaled as ReportBAMread does (KAligner.cpp:6148-6233) */
int k4_format_sam_ext_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                          const void* d_pe, const void* d_seg2, const void* d_reads, const void* d_offs, const void* d_lens,
                          const k4_sam_names* names, void** d_sam, uint64_t* sam_bytes, k4_sam_stats* stats,
                          uint8_t* chrom_hit, void* stream);
/* k4_format_sam_all_dev <- kalign -M1 (eFMsamAll; WriteBAMReadHits KAligner.cpp:5846-5866, the unaligned branch of ReportBAMread
 * :6253-6276): the same body followed by one record per loaded read that was not accepted, grouped by NAR code in ascending order
 * (SortHitMatch sorts on NAR first; within a code the reference's order is undefined, here load order):
 * QNAME FLAG(4; PE: 1|2|64/128|4 and the mate's 8 or 32) * 0 128 <len>M * 0 0 SEQ(as read) * <empty field> YU:Z:<two-letter NAR> */
int k4_format_sam_all_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                          const void* d_pe, const void* d_seg2, const void* d_reads, const void* d_offs, const void* d_lens,
                          const k4_sam_names* names, void** d_sam, uint64_t* sam_bytes, k4_sam_stats* stats,
                          uint8_t* chrom_hit, void* stream);
/* ... as BAM records: refID, pos and the mate fields -1, bin 0, MAPQ 128, one CIGAR operation <len>M, aux YU:Z:<NAR> */
int k4_format_bam_all_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                          const void* d_pe, const void* d_seg2, const void* d_reads, const void* d_offs, const void* d_lens,
                          const k4_sam_names* names, int32_t sq_all, void** d_bam, uint64_t* bam_bytes, k4_sam_stats* stats,
                          uint8_t* chrom_hit, void* stream);
/* k4_unaligned_fasta_dev <- kalign -j / -J (CKAligner::ReportNoneAligned / ReportMultiAlign, KAligner.cpp:3833-4020): the loaded reads
 * whose NAR is EN or NL (which 0) / ML (which 1) as FASTA, `>lcl|na|<ReadID> <name> <ReadID>|1|<len>` (`lcl|ml` for which 1; ReadID
 * 1.. over the loaded reads in load order) and the read as loaded at 70 bases per line, grouped by NAR.  *text: malloc'd host text
 * (k4_free_host). */
int k4_unaligned_fasta_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_pe, const void* d_reads,
                           const void* d_offs, const void* d_lens, const k4_sam_names* names, int32_t which, char** text,
                           uint64_t* text_bytes, uint64_t* n_listed, void* stream);
/* k4_format_bam_dev <- the same alignments as uncompressed BAM records in coordinate order (CSAMfile::AddAlignment's BAM branch,
 * SAMfile.cpp:2379-2640: block_size, refID, pos, bin<<16|MAPQ<<8|l_read_name, FLAG<<16|n_cigar_op, l_seq, next_refID,
 * next_pos, tlen, read_name, cigar, 4-bit seq -- reverse complemented for a Crick alignment --, qual 0xff).  refID is the
 * index in the header's reference dictionary: every sequence of the index when sq_all, else those that received a hit, in
 * index order (WriteBAMReadHits, KAligner.cpp:5785-5821).  Magic, header text, dictionary, BGZF blocks and the .bai index
 * are the caller's (include/k4_bam.hpp does them on host threads). */
int k4_format_bam_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                      const void* d_pe, const void* d_seg2, const void* d_reads, const void* d_offs, const void* d_lens,
                      const k4_sam_names* names, int32_t sq_all, void** d_bam, uint64_t* bam_bytes, k4_sam_stats* stats,
                      uint8_t* chrom_hit, void* stream);
/* k4_snp_csv_dev <- CKAligner::ProcessSNPs + OutputSNPs (KAligner.cpp:8168-8590, 7098-7760; `kalign -p<n> -P<q> -S<file>`): SNP calls
 * over the accepted alignments of a run, as the text of kalign's main SNP CSV (header line included).  Per chromosome on the
 * device: base counts per locus, the 51-base background window, the coverage / non-reference tests; on the host, for the loci that
 * pass: binomial p-value (CStats::Binomial), Benjamini-Hochberg at `qvalue`, ranks, text.  min_snp_reads: kalign -p (1..),
 * snp_nonref_pcnt: kalign -1 (percent).  *csv is malloc'd: release with k4_free_host.  The files kalign writes beside the CSV
 * (coverage WIG, DiSNPs, TriSNPs, markers, centroids) come from k4_snp_files_dev / k4_snp_run_dev / k4_snp_run2_dev. */
int k4_snp_csv_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml, const void* d_pe,
                   const void* d_reads, const void* d_offs, const void* d_lens, int32_t min_snp_reads, double qvalue,
                   double snp_nonref_pcnt, char** csv, uint64_t* csv_bytes, uint64_t* n_snps, void* stream);
/* ... as VCF 4.1 (what kalign writes when the SNP file's name ends in .vcf): ALT = the alleles with at least a tenth of the strongest
 * one's count, AF per allele, QUAL = phred of the p-value capped at 100, DP = coverage */
int k4_snp_vcf_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml, const void* d_pe,
                   const void* d_reads, const void* d_offs, const void* d_lens, int32_t min_snp_reads, double qvalue,
                   double snp_nonref_pcnt, char** vcf, uint64_t* vcf_bytes, uint64_t* n_snps, void* stream);
/* both files of a kalign SNP run: the SNP file (vcf == 0: CSV) and the coverage WIG kalign writes beside it (<snp file minus its
 * extension>.covsegs.wig: variableStep spans of roughly equal coverage, AccumWIGCnts / CompleteWIGSpan KAligner.cpp:6993-7085;
 * walked on host threads, one per chromosome, while the device piles up the next ones) */
int k4_snp_files_dev(k4_index* ix, int vcf, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                     const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens, int32_t min_snp_reads, double qvalue,
                     double snp_nonref_pcnt, char** snp, uint64_t* snp_bytes, uint64_t* n_snps, char** wig, uint64_t* wig_bytes,
                     void* stream);
/* every file of a kalign SNP run: the two above and the haplotype files kalign writes beside them (<snp file minus its extension>
 * .disnp.csv / .trisnp.csv, KAligner.cpp:4553-4554, header :8252-8330, lines :7767-8101: two / three called loci following each
 * other within min(300, mean aligned length) bases, the alignments covering all of them (IterateReadsOverlapping :10475-10546)
 * and how many show each base combination (AdjAlignSNPBase :1581-1632)).  Each text is malloc'd: release with k4_free_host. */
typedef struct k4_snp_files {
  char* snp;    uint64_t snp_bytes;  uint64_t n_snps;
  char* wig;    uint64_t wig_bytes;
  char* disnp;  uint64_t disnp_bytes;
  char* trisnp; uint64_t trisnp_bytes;
} k4_snp_files;
int k4_snp_run_dev(k4_index* ix, int vcf, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                   const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens, int32_t min_snp_reads, double qvalue,
                   double snp_nonref_pcnt, k4_snp_files* out, void* stream);
/* ... and the two files kalign writes from the same per-locus counts when asked to:
 *   markers (kalign -K<len> [--markerpolythres <dbl>], KAligner.cpp:7494-7560; the file is <snp file>.markers): for every candidate
 *   locus that passed the background noise test, the marker_len (0: none, else 25..500) consensus bases around it, marker_len / 2
 *   in front.  A candidate too close to an end, with a non-reference proportion below 0.5, with a marker locus covered by fewer
 *   than min_snp_reads bases or too polymorphic (k4_marker_classify_host has that rule), or whose centre calls the reference base
 *   has no marker and is DROPPED before the p-values and the Benjamini-Hochberg cut: ranks, calls, DiSNPs / TriSNPs and the WIG's
 *   last span all follow.  An accepted one gets the next marker id of the run, a FASTA record
 *   ">Marker<id> <chrom> <start>|<len>|<locus>|<len / 2>|<SNP base>|<ref base>|<polymorphic sites>" whether or not it is called later,
 *   and its id and polymorphic site count in the CSV's last two columns.
 *   centroids (kalign -7 <file>, :7380-7398, :8104-8133, :8626-8660): a CSV of all 4^7 7-mers, one line each: how many loci with at
 *   least min_snp_reads bases have it as the reference sequence around them (3 bases either side, no non-ACGT symbol; counted on
 *   the device over every locus of every sequence with alignments, independent of calling), how many called SNPs, and the sums of
 *   those SNPs' reference count and five non-reference counts as piled.  Counts are kept in 64 bits and printed as int, as the
 *   reference prints them.
 * Without either option the four texts are those of k4_snp_run_dev; markers / centroids stay NULL unless asked for.  Each text is
 * malloc'd: release with k4_free_host. */
typedef struct k4_snp_opts {
  int32_t marker_len;        /* kalign -K: 0 or 25..500 */
  int32_t want_centroids;    /* kalign -7 */
  double marker_poly_thres;  /* kalign --markerpolythres: 0.0..0.5 (kalign's default: 1.0 / 3.0) */
} k4_snp_opts;
typedef struct k4_snp_files2 {
  k4_snp_files files;
  char* markers;   uint64_t markers_bytes;  uint64_t n_markers;
  char* centroids; uint64_t centroids_bytes;
} k4_snp_files2;
int k4_snp_run2_dev(k4_index* ix, int vcf, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml,
                    const void* d_pe, const void* d_reads, const void* d_offs, const void* d_lens, int32_t min_snp_reads, double qvalue,
                    double snp_nonref_pcnt, const k4_snp_opts* opts, k4_snp_files2* out, void* stream);
/* the marker rule of one locus alone, on the host (no device, no index): the same function the kernel runs.  cnt7 / ref_bases as for
 * k4_pba_classify_host.  tot = ref + nonref; tot < min_snp_reads: base 0xff (the marker is rejected).  nonref / (double)tot <=
 * poly_thres: the target's base, polymorphic when that proportion > 0.1.  Else the first of A, C, G, T, N with a count > 0 and
 * count / (double)tot >= 1.0 - poly_thres: that base (0..4), polymorphic when its proportion < 0.9; none: base 0xfe (rejected). */
int k4_marker_classify_host(const uint32_t* cnt7, uint64_t stride, uint32_t n_loci, const uint8_t* ref_bases, int32_t min_snp_reads,
                            double poly_thres, uint8_t* base, uint8_t* poly);
void k4_free_host(void* p);
/* k4_pba_run_dev <- `ngskit4b genpba` (kalignerPBA, KAlignerCL.cpp:1540-2290: CKAligner::Process with eFMPBA; ProcessSNPs
 * KAligner.cpp:8168-8575 and the PBA branch of OutputSNPs :7194-7317): the packed base alleles of a run's accepted alignments and
 * the coverage WIG genpba writes beside them (<out minus its extension>.covsegs.wig).  pba: the text
 * "Type:PbA\nVersion:1\nExperimentID:<experiment_id>\nReferenceID:<the index's species>\nReadsetID:<readset_id>" and a NUL, then per
 * sequence with a piled-up alignment, in sequence order: one byte name length, the name, a NUL, the sequence length (uint32, little
 * endian) and one byte per locus -- four 2-bit allele scores, A in bits 7..6, C in 5..4, G in 3..2, T in 1..0 (k4_pba_classify_host
 * has the rule).  No such sequence: pba_bytes == 0, as the reference leaves an empty file.  wig: no track line, the loci counted
 * from 1, coverage without the indeterminate bases, every sequence's last span closed.  Alignments with an indel or a splice
 * junction and those reaching over their sequence's end are left out, as in SNP calling.  Both blocks are malloc'd: release with
 * k4_free_host.  The ids are written as they are (k4align cleans them as the reference's front end does). */
typedef struct k4_pba_files {
  uint8_t* pba; uint64_t pba_bytes;
  char* wig;    uint64_t wig_bytes;
  uint64_t n_chroms;
} k4_pba_files;
int k4_pba_run_dev(k4_index* ix, int pe, int64_t n_units, const void* d_rr, const void* d_hits, int32_t max_ml, const void* d_pe,
                   const void* d_reads, const void* d_offs, const void* d_lens, const char* experiment_id, const char* readset_id,
                   k4_pba_files* out, void* stream);
/* genpba's per-locus rule alone, on the host (no device, no index): the same function the kernel runs.  cnt7: seven arrays of
 * `stride` words (NumRefBases, NumNonRefBases, NonRefBaseCnts[A, C, G, T, N]); ref_bases: the target's symbol per locus (0..3 =
 * a, c, g, t).  coverage = ref + nonref - N; byte 0 where it is 0; else per allele its count (the reference count for the target's
 * base) / (double)coverage scored 3 / 2 / 1 from 0.75 / 0.35 / 0.20 on where coverage >= 5, and 2 / 1 from 0.70 / 0.30 on below. */
int k4_pba_classify_host(const uint32_t* cnt7, uint64_t stride, uint32_t n_loci, const uint8_t* ref_bases, uint8_t* pba, uint32_t* coverage);
/* k4_select_hits_dev <- MLMode eMLrand (`-r2`, KAligner.cpp:9945-9962) after k4_kalign_batch_dev with pe_mode 2: every accepted
 * read keeps ONE instance, hits[choice[i] % NumHits] moved to slot 0, NumHits = 1.  d_choice: uint32 per read, the caller's
 * draws (the reference: rand() once per read within the limit, in load order when it runs one thread). */
int k4_select_hits_dev(k4_index* ix, int64_t n_reads, int32_t max_ml, void* d_rr, void* d_hits, const void* d_choice,
                       void* stream);
/* k4_assign_multi_dev <- CKAligner::AssignMultiMatches (KAligner.cpp:5092-5258; scoring: ProcAssignMultiMatches :4944-5085),
 * MLMode eMLuniq (ml_mode 3, `-r3`) / eMLmulti (4, `-r4`), after k4_kalign_batch_dev with pe_mode 1 over ALL reads of the
 * run (the clustering is global): a multi-aligned read whose best locus clusters well enough with other reads (score >= 50
 * and twice the next locus') becomes accepted with that locus in slot 0 (NumHits 1, LowHitInstances 1).
 * max_reads_len: the longest read loaded (m_MaxReadsLen).  Waits for `stream`. */
int k4_assign_multi_dev(k4_index* ix, int ml_mode, int32_t max_reads_len, int64_t n_reads, int32_t max_ml, void* d_rr,
                        void* d_hits, int64_t* n_assigned, void* stream);
/* ---- the overlapped host <-> device pipeline (kit4b_amd/csrc/k4_pipeline.hip) ---------------------------
 * <- the reference's loader thread running beside its aligner threads (CKAligner::InitiateLoadingReads / ProcLoadReadFiles,
 *    KAligner.cpp:4786-4866,11323-11496; ThreadedIterReads :10370-10438) and its writer (WriteBAMReadHits :5718).
 * Three HIP streams: the caller's reader thread(s) fill pinned ring buffers (k4_pipeline_acquire / _submit) whose contents go
 * up on the copy stream while a worker thread of the library parses, filters and aligns the chunks that have already arrived
 * on the compute stream; k4_pipeline_format then makes ONE coordinate-sorted SAM body over everything (identical to a single
 * batch), which k4_pipeline_next_sam hands out piece by piece from a second pinned ring while the next pieces come down.
 * One acquire, then one submit, per end at a time; `final` marks the last chunk of an end (bytes may be 0). */
typedef struct k4_pipeline k4_pipeline;
typedef struct {
  int32_t paired;               /* 0: one input (SE), 1: two inputs, record i of end 0 pairs with record i of end 1 */
  k4_kalign_params kp;          /* as for k4_kalign_ext_batch_dev / k4_kalign_pe_batch_dev (PE: max_ml 10, pe_mode 1) */
  k4_pe_params pe;
  int32_t min_len, max_len;     /* the length filter of LoadRawReads (k4_prepare_reads_dev) */
  uint32_t n_buffers;           /* pinned buffers per end (0: 3) */
  uint32_t min_batch_units;     /* reads / pairs that must have arrived before an alignment batch is launched (0: 2^22; not
                                 * over the last eighth of an input whose size is known: little is left behind the last upload) */
  uint64_t chunk_bytes;         /* size of one pinned buffer = one upload (0: 256 MiB) */
  uint64_t expect_text_bytes[2];/* text per end, if known (file sizes): the HBM arena is sized once */
} k4_pipeline_params;
typedef struct {                /* where the aligned batch lives in HBM (for the global stages between alignment and report:
                                 * k4_assign_multi_dev, k4_select_hits_dev, k4_auto_trim_flanks_dev, k4_remove_orphan_juncts_dev) */
  int64_t n_units, n_reads;     /* reads (SE) / pairs (PE); reads through the SE pass */
  uint32_t max_read_len;
  int32_t max_ml;
  uint64_t n_under, n_over;     /* sloughed by the length filter */
  void *d_rr, *d_hits, *d_seg2, *d_pe, *d_reads, *d_offs, *d_lens;
  k4_sam_names names;
} k4_pipeline_view;
int k4_pipeline_open(k4_index* ix, const k4_pipeline_params* p, k4_pipeline** out);
int k4_pipeline_set_trims(k4_pipeline* pl, int32_t trim5, int32_t trim3); /* kalign -y / -Y; before the first chunk is submitted */
int k4_pipeline_set_sampling(k4_pipeline* pl, int32_t sample_nth);          /* kalign -#<n> (one input file per end); likewise */
/* kalign -H: k4_contam_trims_dev runs on the compute stream between the parse and the prepare of every batch (the table, a HOST array
 * of k4_load_contaminants, is copied); likewise before the first chunk.  Never called: no kernel more, no buffer more than before */
int k4_pipeline_set_contaminants(k4_pipeline* pl, const k4_contaminant* tbl, int32_t n);
/* ... and after k4_pipeline_wait_aligned the reference's four totals (n_contam4 of k4_prepare_reads_contam_dev) over the run */
int k4_pipeline_contam_totals(k4_pipeline* pl, uint64_t* n_contam4);
int k4_pipeline_acquire(k4_pipeline* pl, int end, void** buf, uint64_t* cap); /* blocks while every buffer is on its way up */
int k4_pipeline_submit(k4_pipeline* pl, int end, uint64_t bytes, int final_chunk);
/* text in the caller's own memory (pinned for the full PCIe rate); it must stay valid until k4_pipeline_wait_aligned returns */
int k4_pipeline_submit_host(k4_pipeline* pl, int end, const void* text, uint64_t bytes, int final_chunk);
int k4_pipeline_wait_aligned(k4_pipeline* pl, k4_pipeline_view* view); /* after the final chunks: every read is aligned */
/* k4_align_stats_dev over the pipeline's own arrays; call it behind the last global stage and before k4_pipeline_format* */
int k4_pipeline_align_stats(k4_pipeline* pl, k4_align_stats* out);
/* k4_site_prefs_dev over the pipeline's own arrays; likewise behind the last global stage and before k4_pipeline_format* */
int k4_pipeline_site_prefs(k4_pipeline* pl, int32_t ofs, k4_site_prefs* out);
/* k4_pe_insert_dist_dev over a paired-end pipeline's own arrays; likewise */
int k4_pipeline_pe_insert_dist(k4_pipeline* pl, k4_pe_insert_dist* out);
int k4_pipeline_format(k4_pipeline* pl, k4_sam_stats* stats, uint8_t* chrom_hit /* host, n_entries + 1, or NULL */, uint64_t* sam_bytes);
/* ... as BAM records (k4_format_bam_dev); the pieces come down through k4_pipeline_next_sam / k4_pipeline_read_sam all the same */
int k4_pipeline_format_bam(k4_pipeline* pl, int32_t sq_all, k4_sam_stats* stats, uint8_t* chrom_hit, uint64_t* bam_bytes);
/* ... as SAM text with every loaded read (k4_format_sam_all_dev, kalign -M1) */
int k4_pipeline_format_all(k4_pipeline* pl, k4_sam_stats* stats, uint8_t* chrom_hit, uint64_t* sam_bytes);
int k4_pipeline_format_bam_all(k4_pipeline* pl, int32_t sq_all, k4_sam_stats* stats, uint8_t* chrom_hit, uint64_t* bam_bytes);
int k4_pipeline_next_sam(k4_pipeline* pl, const void** ptr, uint64_t* bytes); /* valid until the next call; 0 bytes: done */
int k4_pipeline_read_sam(k4_pipeline* pl, void* dst, uint64_t cap, uint64_t* bytes); /* the whole body into caller memory */
void k4_pipeline_close(k4_pipeline* pl);

void k4_free_device(void* p);
/* device memory for host programs that use the *_dev entry points without a HIP runtime of their own */
int k4_alloc_device(k4_index* ix, uint64_t bytes, void** d_ptr);
int k4_copy_to_device(k4_index* ix, void* d_dst, const void* src, uint64_t bytes);
int k4_copy_to_host(k4_index* ix, void* dst, const void* d_src, uint64_t bytes);
/* pageable or file-mapped host memory -> device memory through pinned pieces filled by several host threads (the way k4_open
 * itself uploads the two big arrays of an .sfx file); for callers that place an index themselves, e.g. libk4comm's rank 0 */
int k4_upload_pageable(int device, void* d_dst, const void* h_src, uint64_t bytes);
/* the caller's own host memory (page-aligned address and length, e.g. a mapped file) registered with the HIP runtime in place, so
 * that the device copies of the *_dev / pipeline entry points run from / into it at the full PCIe rate without a staging copy */
int k4_host_register(void* p, uint64_t bytes);
int k4_host_unregister(void* p);

/* kernel timing for roofline measurement: when enabled, every batch brackets the dominant kernel (k4k_align_step, one launch per AlignReads phase) with
 * HIP events on the stream it is launched on; k4_get_kernel_times synchronises, returns the summed duration and the
 * number of launches since the last call, and resets. */
int k4_enable_kernel_timing(k4_index* ix, int on);
int k4_get_kernel_times(k4_index* ix, double* fast_kernel_ms, int32_t* launches);
/* ... both parts of a batch: the step kernels (as above) and the general kernel's passes (k4k_align_slow) that follow them on
 * the same stream; their sum is the device time of the batch's alignment */
int k4_get_kernel_times_split(k4_index* ix, double* step_kernels_ms, double* general_kernel_ms, int32_t* launches);
int k4_get_counters(k4_index* ix, k4_counters* out); /* synchronises the device */
int k4_reset_counters(k4_index* ix);
int k4_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
