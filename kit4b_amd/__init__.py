"""kit4b_amd -- MI355X-native kit4b kalign hot path (seed lookup + mismatch-bounded extension).

This package is a thin ctypes binding over the C ABI of ``kit4b_amd/libk4sfx.so`` (include/k4sfx.h), which holds
the hand-written HIP kernels for gfx950.  It exists for the tests and bench.py; the product boundary is the C ABI
and the C++ ``CSfxArray`` facade in include/k4_sfxarray.hpp.  There is no CPU fallback: importing works anywhere,
every compute call needs the library and a GPU and raises ``K4Error`` otherwise.
"""
import bisect
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, os.environ.get("K4SFX_LIB_NAME", "libk4sfx.so"))  # (the override: development builds, tools/slow_prof.py)

STRAND_BOTH, STRAND_WATSON, STRAND_CRICK = 0, 1, 2
HR_NONE, HR_HITS, HR_MMDELTA, HR_HITINSTS, HR_RMMDELTA, HR_SEQERRS = 0, 1, 2, 3, 4, 5
NAR_ACCEPTED, NAR_NS, NAR_NOHIT, NAR_MMDELTA, NAR_MULTIALIGN = 1, 2, 3, 4, 5

HIT_DTYPE = np.dtype(
    [("chrom_id", "<u4"), ("match_loci", "<u4"), ("match_len", "<u2"), ("strand", "u1"), ("mismatches", "u1"),
     ("reserved", "<u4")]
)
RESULT_DTYPE = np.dtype(
    [("hit_rslt", "<i4"), ("inst", "<i4"), ("low_mm", "<i4"), ("nxt_mm", "<i4"), ("nar", "<i4"), ("num_hits", "<i4")]
)
# k4_hit.ext (the dtype's "reserved" word): TrimLeft | TrimRight << 12 | K4_EXT_*; k4_seg2: Seg[1] of a two-segment hit
EXT_CHIMERIC, EXT_INDEL, EXT_INSERT, EXT_SPLICE, EXT_NONORPHAN = 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28
SEG2_DTYPE = np.dtype(
    [("chrom_id", "<u4"), ("match_loci", "<u4"), ("match_len", "<u2"), ("read_ofs", "<u2"), ("mismatches", "u1"),
     ("reserved", "u1"), ("score", "<u2")]
)
NAR_TRIM, NAR_SPLICEJCTN, NAR_MICROINDEL, NAR_PCRDUP = 6, 7, 8, 9


class K4Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("k4sfx error %d: %s" % (code, msg))
        self.code = code


class Entry(C.Structure):
    _fields_ = [("entry_id", C.c_uint32), ("fblock_id", C.c_uint32), ("name", C.c_char * 81),
                ("name_hash", C.c_uint16), ("seq_len", C.c_uint32), ("start_ofs", C.c_uint64),
                ("end_ofs", C.c_uint64)]


class Info(C.Structure):
    _fields_ = [("concat_len", C.c_uint64), ("tot_seqs_len", C.c_uint64), ("sfx_el_size", C.c_uint32),
                ("n_entries", C.c_uint32), ("kmer_k", C.c_uint32), ("n_exc_blocks", C.c_uint32),
                ("device_bytes", C.c_uint64), ("device", C.c_int32), ("max_iter", C.c_int32),
                ("dataset", C.c_char * 81)]


class AlignParams(C.Structure):
    _fields_ = [("tot_mm", C.c_int32), ("core_len", C.c_int32), ("core_delta", C.c_int32),
                ("max_core_slides", C.c_int32), ("min_core_len", C.c_int32), ("mm_delta", C.c_int32),
                ("strand", C.c_int32), ("max_hits", C.c_int32), ("min_chimeric_len", C.c_int32),
                ("micro_indel_len", C.c_int32), ("max_splice_junct_len", C.c_int32)]


class KalignParams(C.Structure):
    _fields_ = [("max_subs", C.c_int32), ("min_edit_dist", C.c_int32), ("max_ns", C.c_int32), ("pmode", C.c_int32),
                ("strand", C.c_int32), ("max_ml", C.c_int32), ("pe_mode", C.c_int32), ("min_core_len", C.c_int32),
                ("max_num_slides", C.c_int32), ("min_chimeric_len", C.c_int32), ("micro_indel_len", C.c_int32),
                ("max_splice_junct_len", C.c_int32)]


class PeParams(C.Structure):
    _fields_ = [("pe_mode", C.c_int32), ("pair_min_len", C.c_int32), ("pair_max_len", C.c_int32),
                ("pair_strand", C.c_int32)]


PE_READ_DTYPE = np.dtype(
    [("nar", "<i4"), ("num_hits", "<i4"), ("inst", "<i4"), ("low_mm", "<i4"), ("pe_aligned", "<i4"), ("rescued", "<i4"),
     ("hit", HIT_DTYPE)]
)


class ParseInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("consumed", C.c_uint64), ("n_bases", C.c_uint64), ("max_len", C.c_uint32),
                ("format", C.c_uint32)]


class SamNames(C.Structure):
    _fields_ = [("d_text", C.c_void_p * 2), ("d_name_off", C.c_void_p * 2), ("d_name_len", C.c_void_p * 2)]


class SamStats(C.Structure):
    _fields_ = [("nar", C.c_uint64 * 20), ("plus", C.c_uint64), ("minus", C.c_uint64), ("n_lines", C.c_uint64)]


FASTA, FASTQ = 1, 2


class PipelineParams(C.Structure):
    _fields_ = [("paired", C.c_int32), ("kp", KalignParams), ("pe", PeParams), ("min_len", C.c_int32), ("max_len", C.c_int32),
                ("n_buffers", C.c_uint32), ("min_batch_units", C.c_uint32), ("chunk_bytes", C.c_uint64),
                ("expect_text_bytes", C.c_uint64 * 2)]


class PipelineView(C.Structure):
    _fields_ = [("n_units", C.c_int64), ("n_reads", C.c_int64), ("max_read_len", C.c_uint32), ("max_ml", C.c_int32),
                ("n_under", C.c_uint64), ("n_over", C.c_uint64), ("d_rr", C.c_void_p), ("d_hits", C.c_void_p),
                ("d_seg2", C.c_void_p), ("d_pe", C.c_void_p), ("d_reads", C.c_void_p), ("d_offs", C.c_void_p),
                ("d_lens", C.c_void_p), ("names", SamNames)]


class LociConstraint(C.Structure):  # k4_loci_constraint
    _fields_ = [("chrom_id", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("bits", C.c_uint8), ("reserved", C.c_uint8 * 3)]


LOCI_CONSTRAINT_DTYPE = np.dtype([("chrom_id", "<u4"), ("start", "<u4"), ("end", "<u4"), ("bits", "u1"), ("reserved", "u1", (3,))])
NAR_CHROMFILT, NAR_LOCICONSTRAINED = 11, 19


class Contaminant(C.Structure):  # k4_contaminant
    _fields_ = [("cls", C.c_uint8), ("len", C.c_uint8), ("revcpl", C.c_uint8), ("reserved", C.c_uint8 * 5), ("p0", C.c_uint64 * 4),
                ("p1", C.c_uint64 * 4), ("nmask", C.c_uint64 * 4)]


CONTAMINANT_DTYPE = np.dtype([("cls", "u1"), ("len", "u1"), ("revcpl", "u1"), ("reserved", "u1", (5,)), ("p0", "<u8", (4,)), ("p1", "<u8", (4,)),
                              ("nmask", "<u8", (4,))])
CONTAM_5PE1, CONTAM_5PE2, CONTAM_3PE1, CONTAM_3PE2 = 0, 1, 2, 3  # teContamType


class AlignStats(C.Structure):  # k4_align_stats
    _fields_ = [("max_align_len", C.c_uint32), ("len_stride", C.c_uint32), ("n_entries", C.c_uint32), ("reserved", C.c_uint32),
                ("n_accepted", C.c_uint64), ("q_insts", C.POINTER(C.c_uint64)), ("q_subs", C.POINTER(C.c_uint64)),
                ("m_sub", C.POINTER(C.c_uint64)), ("multi_hit", C.POINTER(C.c_uint64)), ("pe_len_dist", C.POINTER(C.c_uint64)),
                ("ent_hits", C.POINTER(C.c_uint32)), ("ent_uniq_loci", C.POINTER(C.c_uint32)),
                ("ent_indeterminate", C.POINTER(C.c_uint32)), ("ent_trimer", C.POINTER(C.c_uint32)), ("block", C.c_void_p)]


STATS_MULTI, STATS_PE_LEN = 500, 100000


class SitePrefs(C.Structure):  # k4_site_prefs
    _fields_ = [("num_occs", C.POINTER(C.c_uint32) * 2), ("num_sites", C.POINTER(C.c_uint32) * 2), ("n_accepted", C.c_uint64),
                ("n_counted", C.c_uint64), ("block", C.c_void_p)]


class PeInsertDist(C.Structure):  # k4_pe_insert_dist
    _fields_ = [("n_rows", C.c_uint32), ("reserved", C.c_uint32), ("entry_id", C.POINTER(C.c_uint32)), ("tot_pes", C.POINTER(C.c_uint32)),
                ("median", C.POINTER(C.c_uint32)), ("sum", C.POINTER(C.c_uint64)), ("dist", C.POINTER(C.c_uint32)), ("block", C.c_void_p)]


PE_INSERT_BINS = 52


class PbaFiles(C.Structure):  # k4_pba_files
    _fields_ = [("pba", C.c_void_p), ("pba_bytes", C.c_uint64), ("wig", C.c_void_p), ("wig_bytes", C.c_uint64), ("n_chroms", C.c_uint64)]


class Counters(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_lookup", C.c_uint64), ("n_probe", C.c_uint64), ("n_cand", C.c_uint64),
                ("n_slow", C.c_uint64), ("n_bases", C.c_uint64)]


class SnpFiles(C.Structure):  # k4_snp_files
    _fields_ = [("snp", C.c_void_p), ("snp_bytes", C.c_uint64), ("n_snps", C.c_uint64), ("wig", C.c_void_p), ("wig_bytes", C.c_uint64),
                ("disnp", C.c_void_p), ("disnp_bytes", C.c_uint64), ("trisnp", C.c_void_p), ("trisnp_bytes", C.c_uint64)]


class SnpOpts(C.Structure):  # k4_snp_opts
    _fields_ = [("marker_len", C.c_int32), ("want_centroids", C.c_int32), ("marker_poly_thres", C.c_double)]


class SnpFiles2(C.Structure):  # k4_snp_files2
    _fields_ = [("files", SnpFiles), ("markers", C.c_void_p), ("markers_bytes", C.c_uint64), ("n_markers", C.c_uint64),
                ("centroids", C.c_void_p), ("centroids_bytes", C.c_uint64)]


DFLT_MARKER_POLY_THRES = 1.0 / 3.0  # cDfltMinMarkerSNPProp (KAligner.h:73)

_lib = None

# every symbol include/k4sfx.h declares
ABI_SYMBOLS = [
    "k4_open", "k4_open_async", "k4_open_wait", "k4_open_seconds", "k4_open_host", "k4_open_device", "k4_close", "k4_last_error", "k4_global_error", "k4_info",
    "k4_get_entry", "k4_get_ident", "k4_set_max_iter", "k4_set_fastq_quality", "k4_get_seq", "k4_write_sfx", "k4_build_sa_device",
    "k4_reserve", "k4_align_reads_batch", "k4_align_reads_batch_dev", "k4_kalign_batch", "k4_kalign_batch_dev",
    "k4_min_core_len", "k4_get_counters", "k4_reset_counters", "k4_abi_version", "k4_enable_kernel_timing",
    "k4_get_kernel_times", "k4_get_kernel_times_split", "k4_snp_csv_dev", "k4_snp_vcf_dev", "k4_snp_files_dev", "k4_snp_run_dev", "k4_free_host", "k4_format_bam_dev", "k4_format_sam_all_dev", "k4_pipeline_format_bam", "k4_pipeline_format_all", "k4_pipeline_format_bam_all", "k4_format_bam_all_dev", "k4_pipeline_set_trims", "k4_pipeline_set_sampling", "k4_unaligned_fasta_dev", "k4_prepare_reads_trim_dev", "k4_mate_rescue_batch", "k4_kalign_pe_batch", "k4_kalign_pe_batch_dev",
    "k4_parse_fastx_dev", "k4_prepare_reads_dev", "k4_format_sam_dev", "k4_free_device", "k4_alloc_device",
    "k4_copy_to_device", "k4_copy_to_host", "k4_upload_pageable", "k4_host_register", "k4_host_unregister", "k4_best_matches_batch", "k4_best_matches_batch_dev",
    "k4_get_sfx_header", "k4_set_description", "k4_select_hits_dev",
    "k4_assign_multi_dev", "k4_align_reads_ext_batch", "k4_align_reads_ext_batch_dev", "k4_kalign_ext_batch",
    "k4_kalign_ext_batch_dev", "k4_auto_trim_flanks_dev", "k4_remove_orphan_juncts_dev", "k4_reduce_pcr_dups_dev", "k4_pcr5_primer_correct_dev", "k4_format_sam_ext_dev",
    "k4_pipeline_open", "k4_pipeline_acquire", "k4_pipeline_submit", "k4_pipeline_submit_host", "k4_pipeline_wait_aligned",
    "k4_pipeline_format", "k4_pipeline_next_sam", "k4_pipeline_read_sam", "k4_pipeline_close", "k4_sfx_map", "k4_sfx_unmap",
    "k4_set_raw_header", "k4_align_stats_collect", "k4_align_stats_dev", "k4_free_align_stats", "k4_write_align_stats",
    "k4_pipeline_align_stats", "k4_filter_loci_constraints_dev", "k4_filter_chroms_dev", "k4_load_loci_constraints", "k4_chrom_accept_mask",
    "k4_filter_marked_prior", "k4_site_prefs_dev", "k4_free_site_prefs", "k4_write_site_prefs", "k4_pipeline_site_prefs",
    "k4_pe_insert_dist_dev", "k4_free_pe_insert_dist", "k4_write_pe_insert_dist", "k4_pipeline_pe_insert_dist", "k4_pe_insert_bin_host",
    "k4_pe_insert_median_host", "k4_pba_run_dev", "k4_pba_classify_host", "k4_snp_run2_dev", "k4_marker_classify_host",
    "k4_load_contaminants", "k4_contam_match_host", "k4_contam_trims_dev", "k4_prepare_reads_contam_dev", "k4_pipeline_set_contaminants",
    "k4_pipeline_contam_totals", "k4_set_priority_regions", "k4_filter_priority_regions_dev", "k4_priority_times", "k4_priority_select_dev",
    "k4_query_reserve", "k4_locate_query_seqs_batch", "k4_locate_query_seqs_batch_dev", "k4_query_last_kernel_ms",
    "k4_blitz_paths_batch", "k4_blitz_paths_batch_dev", "k4_blitz_last_kernel_ms",
    "k4_locate_sfx_hammings_batch", "k4_locate_sfx_hammings_batch_dev", "k4_locate_hammings_batch", "k4_locate_hammings_batch_dev",
    "k4_hamming_last_kernel_ms",
    "k4_kmer_cults_batch", "k4_kmer_cults_batch_dev", "k4_cults_last_kernel_ms", "k4_get_sfx_els",
    "k4_exact_ranges_batch", "k4_exact_ranges_batch_dev", "k4_matches_other_chroms_batch", "k4_species_kmers_batch",
    "k4_species_kmers_batch_dev", "k4_kmarkers_last_kernel_ms",
    "k4_all_near_matches_batch", "k4_all_near_matches_batch_dev", "k4_zygosity_batch", "k4_zygosity_batch_dev", "k4_zygosity_last_kernel_ms",
]


class HammingParams(C.Structure):  # k4_hamming_params
    _fields_ = [("rhamm", C.c_int32), ("kmer_len", C.c_int32), ("sample_nth", C.c_int32), ("both_strands", C.c_int32),
                ("min_core_depth", C.c_uint32), ("max_core_depth", C.c_uint32), ("intra_inter_both", C.c_int32)]


class KMarkersParams(C.Structure):  # k4_kmarkers_params
    _fields_ = [("kmer_len", C.c_int32), ("min_hamming", C.c_int32), ("mode", C.c_int32), ("prefix_len", C.c_int32),
                ("min_with_prefix", C.c_int32), ("reserved", C.c_int32)]


class KMarkersTotals(C.Structure):  # k4_kmarkers_totals
    _fields_ = [("processed", C.c_uint64), ("cultivar_specific", C.c_uint64), ("hamming_retained", C.c_uint64), ("accepted", C.c_uint64)]


class NearParams(C.Structure):  # k4_near_params
    _fields_ = [("max_tot_mm", C.c_int32), ("core_len", C.c_int32), ("core_delta", C.c_int32), ("max_core_slides", C.c_int32),
                ("max_matches", C.c_int32), ("cur_max_iter", C.c_int32), ("n_ident_nodes", C.c_int32), ("reserved", C.c_int32)]


class ZygosityParams(C.Structure):  # k4_zygosity_params
    _fields_ = [("subseq_len", C.c_int32), ("max_subs", C.c_int32), ("max_ns", C.c_int32), ("max_matches", C.c_int32), ("mode", C.c_int32),
                ("reserved", C.c_int32)]


class ZygosityTotals(C.Structure):  # k4_zygosity_totals
    _fields_ = [("windows", C.c_uint64), ("passed_over", C.c_uint64), ("rejected", C.c_uint64), ("unique", C.c_uint64),
                ("unique_matched", C.c_uint64), ("ordered", C.c_uint64), ("second_launch", C.c_uint64)]


ZYG_PASSED_OVER, ZYG_NOT_UNIQUE, ZYG_UNIQUE, ZYG_UNIQUE_MATCHED = range(4)


def genzygosity_limits(tot_seqs_len, subseq_len=25, max_subs=2, mode=0):
    """(CoreLen, MaxNumSlides, MaxIter) that `genzygosity -l -s -m` asks LocateAllNearMatches with over an index of tot_seqs_len bases
    (genzygosity.cpp:681-697, :998-1027, :1190); index.zygosity derives the same in the library"""
    min_core = (5 if tot_seqs_len < 20000000 else 8 if tot_seqs_len < 250000000 else 10) + (4, 2, 0, 6)[mode]
    return max(min_core, subseq_len // (max_subs + 1)), (4, 6, 8, 3)[mode], (5000, 25000, 50000, 1000)[mode]


def genzygosity_csv(index, subseq_len=25, max_subs=2, max_ns=1, max_matches=5000, mode=0, threshold=0.25):
    """The two files `genzygosity -l -s -n -x -m -z -o -O` writes, as bytes (thresholded, raw): index.zygosity over every entry, then
    on the host the report of genzygosity.cpp:746-771 -- every (source, target) pair in order as "src",Subseqs,"targ",Matrix in
    the raw file, and in the thresholded one, with the proportion appended, the pairs of a source with unique windows whose
    proportion is at least the threshold.  index: a SfxIndex, or anything with zygosity() and entry()."""
    matrix, subseqs, _ = index.zygosity(subseq_len=subseq_len, max_subs=max_subs, max_ns=max_ns, max_matches=max_matches, mode=mode)[:3]
    names = [index.entry(i + 1)["name"] for i in range(matrix.shape[1])]
    thr, raw = [], []
    for s, src in enumerate(names):
        n = int(subseqs[s])
        for t, targ in enumerate(names):
            m = int(matrix[s, t])
            if n > 0 and m / n >= threshold:
                thr.append('"%s",%d,"%s",%d,%1.6f\n' % (src, n, targ, m, m / n))
            raw.append('"%s",%d,"%s",%d\n' % (src, n, targ, m))
    return "".join(thr).encode(), "".join(raw).encode()


KMER_NOT_KMER, KMER_FIRST_FOREIGN, KMER_DUPLICATE, KMER_FOREIGN_HIT, KMER_HAMMING, KMER_PREFIX, KMER_ACCEPTED = range(1, 8)


def kmarkers_fasta(index, cultivar, chrom_names, kmer_len=50, mode=0, prefix_len=None, min_shared=0, min_hamming=2):
    """The marker file `ngskit4b kmarkers -T1 -c cultivar -C chrom_names -k -m -p -s -K` writes, as bytes: the species scan
    (index.species_kmers over the targets in the front end's order, its qsort by stricmp of the names, LocKMers.cpp:587) and on the
    host ReportMarker's records (:192-223), one per accepted K-mer in modes 0 and 2 and per flushed run in mode 1 (:1209-1231: the
    mode the help text calls "no extension" is the one that extends, and a run is written when a later accepted K-mer of the same
    ACGT run starts the next one -- the last run of a sequence never is).
    The front end hands MinHamming and MinWithPrefix to LocKMers in each other's place (genkmarkers.cpp:516 against LocKMers.cpp:525):
    -s (min_shared; modes 0 and 1 leave it at 0) is the Hamming separation that is tested and printed, 0 and 1 testing nothing, and -K
    (min_hamming) is the number of other entries that must share the prefix.  This function does the same, as the recorded files
    require.  index: anything with info(), entry(), get_seq() and species_kmers(), SfxIndex or a restatement."""
    if mode not in (0, 1, 2):
        raise K4Error(-100, "Processing mode '-m%d' specified outside of range 0..2" % mode)
    if mode == 2:
        prefix_len = kmer_len // 2 if prefix_len is None else prefix_len
    else:
        prefix_len, min_shared = 0, 0
    if not 1 <= min_hamming <= 5 or min_shared < 0:
        raise K4Error(-100, "Minimum Hamming separation '-K%d' must be in range 1..5" % min_hamming)
    n_entries = index.info()["n_entries"]
    by_name = {}
    for e in range(1, n_entries + 1):
        by_name.setdefault(index.entry(e)["name"].lower(), index.entry(e))
    names = sorted(chrom_names, key=lambda s: s.lower())
    if any(a.lower() == b.lower() for a, b in zip(names, names[1:])) or any(n.lower() not in by_name for n in names):
        raise K4Error(-100, "a target name twice, or one the index does not hold")
    targets = [by_name[n.lower()] for n in names]
    status, _ = index.species_kmers([t["entry_id"] for t in targets], kmer_len, max(min_shared, 1), mode, prefix_len, min_hamming)
    out, base, n_markers = [], 0, 0

    def report(t, loc, length):
        nonlocal n_markers
        n_markers += 1
        seq = index.get_seq(t["entry_id"], loc, min(length, 4000))
        out.append(">%sM%d %d|%d|%d\n%s\n" % (cultivar, n_markers, len(seq), kmer_len, min_shared, "".join("ACGTN"[min(int(b) & 0x0F, 4)] for b in seq)))

    for t in targets:
        st = status[base:base + t["seq_len"]]
        base += t["seq_len"]
        acc = np.flatnonzero(st == KMER_ACCEPTED)
        if mode != 1:
            for loc in acc:
                report(t, int(loc), kmer_len)
            continue
        run_start = prev = None
        for loc in (int(x) for x in acc):
            new_seq = prev is None or (st[prev:loc] == KMER_NOT_KMER).any()  # (K - 1 such bytes end every ACGT run)
            if not new_seq and loc > prev + 1:
                report(t, run_start, kmer_len + prev - run_start)
            if new_seq or loc > prev + 1:
                run_start = loc
            prev = loc
    return "".join(out).encode()


class CultsParams(C.Structure):  # k4_cults_params
    _fields_ = [("prefix_len", C.c_int32), ("suffix_len", C.c_int32), ("min_cultivars", C.c_int32), ("sense_only", C.c_int32),
                ("max_window", C.c_int32), ("max_homozygotic", C.c_int32)]


class CultsOut(C.Structure):  # k4_cults_out
    _fields_ = [("kmers", C.c_void_p), ("bases", C.c_void_p), ("dist", C.c_void_p)]


class CultsCaps(C.Structure):  # k4_cults_caps
    _fields_ = [("max_kmers", C.c_uint64), ("max_dist", C.c_uint64)]


class CultsTotals(C.Structure):  # k4_cults_totals
    _fields_ = [("n_located", C.c_int64), ("n_kmers", C.c_uint64), ("n_dist", C.c_uint64), ("next_sfx_idx", C.c_uint64),
                ("done", C.c_int32), ("reserved", C.c_int32)]


CULT_KMER_DTYPE = np.dtype([("head_sfx_idx", "<u8"), ("dist_ofs", "<u8"), ("sense_cnts", "<u4"), ("antisense_cnts", "<u4"),
                            ("num_cultivars", "<u4"), ("reserved", "<u4")])  # k4_cult_kmer
CULT_DIST_DTYPE = np.dtype([("entry_id", "<u4"), ("sense", "<u4"), ("antisense", "<u4")])  # k4_cult_dist


def kmer_cult_thread_range(n_els, sa_at, bases_at, kmer_len, thread_inst, num_threads, start_sfx_idx):
    """CSfxArray::GenKMerCultThreadRange (libkit4b/SfxArray.cpp:2733-2801) over sa_at(i) -> locus and bases_at(locus, n) -> up to n
    codes (fewer at the end of a sequence: what follows is no base).  Returns (rc, end_sfx_idx): -1 on a bad argument, 0 when
    nothing is left for this thread, 1 with the inclusive end -- which, as there, is the first element of the NEXT K-mer."""
    if num_threads < 1 or num_threads > 64 or thread_inst < 1 or thread_inst > num_threads or start_sfx_idx < 0 or start_sfx_idx >= n_els:
        return -1, 0
    if n_els - start_sfx_idx < 50000:
        return 1, n_els - 1
    end = start_sfx_idx + (n_els - start_sfx_idx) // (1 + num_threads - thread_inst)
    if end + 25000 >= n_els:
        return 1, n_els - 1
    psn1 = sa_at(end)
    el1 = [int(b) & 0x0F for b in bases_at(psn1, kmer_len)]
    end += 1
    while end < n_els:
        psn2 = sa_at(end)
        if psn2 + kmer_len >= n_els:
            return 1, end
        el2 = [int(b) & 0x0F for b in bases_at(psn2, kmer_len)]
        for ofs in range(kmer_len):
            a = el1[ofs] if ofs < len(el1) else 0x0F
            b = el2[ofs] if ofs < len(el2) else 0x0E
            if a > 3 or a != b:
                return 1, end
        end += 1
    return 0, 0


def _revcomp_codes(seq):
    return bytes(3 - b if b <= 3 else b for b in reversed(seq))


def kmermarkers_fasta(index, kmer_len, prefix_len=None, min_shared=0, sense_only=False, threads=1):
    """`ngskit4b kmermarkers -S0` as text: the sweep (index.kmer_cult_thread_range / index.kmer_cults per thread range, as
    CMarkerKMers::LocKMers partitions it, ngskit4b/MarkerKMers.cpp:449-458), then on the host what LocKMers does with the putative
    markers (:576-664): the sort by sequence, the duplicate / overlap / antisense flags (IsMarkerOverlapping and GetMarkerAntisense
    as written, :690-795), the sort by cultivars and counts, and ReportMarker's records (:237-258) for the unflagged ones.  Python's
    sorts are stable where the reference's qsort leaves ties in no fixed order."""
    prefix_len = kmer_len if prefix_len is None else prefix_len
    suffix_len = kmer_len - prefix_len
    n_entries = index.info()["n_entries"]
    min_with = n_entries if min_shared == 0 or min_shared > n_entries else min_shared
    marks = []  # [seq bytes, sense, antisense, cultivars, flags, id]
    start = 0
    for t in range(threads):
        rc, end = index.kmer_cult_thread_range(prefix_len, t + 1, threads, start)
        if rc < 0:
            raise K4Error(rc, "GenKMerCultThreadRange")
        if rc < 1:
            break
        r = index.kmer_cults(prefix_len, suffix_len, min_with, sense_only=sense_only, start_sfx_idx=start, end_sfx_idx=end)
        for k, b in zip(r["kmers"], r["bases"]):
            marks.append([bytes(b[:prefix_len].tolist()), int(k["sense_cnts"]), int(k["antisense_cnts"]), int(k["num_cultivars"]), 0, len(marks) + 1])
        start = end + 1
    n = len(marks)
    order = list(range(n))
    if n > 1:
        order.sort(key=lambda i: marks[i][0])
        for rank, i in enumerate(order):
            marks[i][5] = rank + 1
        seqs = [marks[i][0] for i in order]

        def find(key, width, self_id):  # the binary search of IsMarkerOverlapping / GetMarkerAntisense: the other marker's place, or None
            lo, hi = 0, n - 1
            while hi >= lo:
                t = (lo + hi) // 2
                c = seqs[t][:width]
                if key == c:
                    if marks[order[t]][5] != self_id:
                        return t
                    for u in (t - 1, t + 1):
                        if 0 <= u < n and seqs[u][:width] == key:
                            return u
                    return None
                if key < c:
                    hi = t - 1
                else:
                    lo = t + 1
            return None

        for idx, i in enumerate(order):
            m = marks[i]
            if idx < n - 1 and seqs[idx + 1] == m[0]:
                m[4] |= 1  # cMarkerDupFlg
            if find(m[0][1:], prefix_len - 1, m[5]) is not None:
                m[4] |= 2  # cMarkerOvlFlg
            if not sense_only:
                t = find(_revcomp_codes(m[0]), prefix_len, m[5])
                if t is not None:
                    anti = marks[order[t]]
                    if anti[5] < m[5] or m[4] & 4:
                        continue
                    if m[4] & 0xFF:
                        m[4] |= 4  # cMarkerAntiFlg
                    else:
                        anti[4] |= 4
        order.sort(key=lambda i: (-marks[i][3], -((marks[i][1] + marks[i][2]) & 0xFFFFFFFF)))
    out, mid = [], 0
    trunc = min(prefix_len, 200)  # cMaxKMerLen
    for i in order:
        m = marks[i]
        if m[4] & 0xFF:
            continue
        mid += 1
        out.append(">KMerM%d %d|%d|%d|%d|%d\n%s\n" % (mid, trunc, kmer_len, m[3], m[1], m[2], "".join("ACGTN"[min(b, 4)] for b in m[0][:trunc])))
    return "".join(out)


HAMMING_DEPTHS = ((200, 5000), (1000, 10000), (2000, 20000), (5000, 50000))  # eSensLess, Default, More, Ultra (hammings.cpp:2366-2386)


def hamming_spans(entry_lens, kmer_len):
    """The spans RestrictedHammingThread (ngskit4b/hammings.cpp:1600-1656) hands to LocateSfxHammings, in its order: (entry_id,
    entry_loci, span_len, out_offs) arrays over one byte array that covers all entries.  MaxHammSeqLen = max(10000, total / 10000);
    the next span starts 1 + CurSeqLen - KMerLen further on; an entry shorter than a K-mer gets none."""
    total = int(sum(int(v) for v in entry_lens))
    max_len = max(10000, total // 10000)
    rows, base = [], 0
    for eid, ln in enumerate((int(v) for v in entry_lens), 1):
        if ln >= kmer_len:
            ofs = 0
            while True:
                cur = min(max_len, ln - ofs)
                rows.append((eid, ofs, cur, base + ofs))
                ofs += 1 + cur - kmer_len
                if ofs + kmer_len > ln:
                    break
        base += ln
    a = np.array(rows, dtype=np.uint64).reshape(-1, 4)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32), a[:, 3].astype(np.uint64)


def hammings_csv(names, entry_lens, hammings, kmer_len):
    """ReportRestrictedHammingsCSV (ngskit4b/hammings.cpp:1772-1833) over the byte array restricted_hammings returns, as text: runs of
    equal bytes per entry.  As there, the run loop compares byte 0 with itself first and never reads the byte of the last K-mer.  Host
    side; no founder prefix."""
    out = ['"Chrom","StartLoci","Len","Hamming"\n']
    base = 0
    for name, ln in zip(names, (int(v) for v in entry_lens)):
        h = hammings[base:base + ln]
        base += ln
        if ln < kmer_len:
            continue
        cur_len, cur, cur_loci, k = 0, int(h[0]), 0, 0
        for loci in range(1, ln - kmer_len + 1):
            v = int(h[k])
            k += 1
            if v == cur:
                cur_len += 1
                continue
            out.append('"%s",%d,%d,%d\n' % (name, cur_loci, cur_len, cur))
            cur_len, cur, cur_loci = 1, v, loci
        out.append('"%s",%d,%d,%d\n' % (name, cur_loci, cur_len, cur))
    return "".join(out)


class QueryParams(C.Structure):  # k4_query_params
    _fields_ = [(n, C.c_int32) for n in ("core_len", "core_delta", "strand", "max_hits", "max_iter", "match_pts", "mismatch_pts")]


QUERY_NODE_DTYPE = np.dtype([(n, "<u4") for n in ("query_start", "align_len", "targ_seq_id", "targ_loci", "n_mismatches", "slot", "strand")])  # k4_query_node


class BlitzParams(C.Structure):  # k4_blitz_params
    _fields_ = [(n, C.c_int32) for n in ("match_pts", "mismatch_pts", "gap_open", "min_path_score", "query_len_aligned_pct", "max_paths", "strand")]


BLITZ_PATH_DTYPE = np.dtype([(n, "<u4") for n in ("query", "targ_seq_id", "strand", "score", "matches", "mismatches", "n_count", "q_num_insert",
                                                  "q_base_insert", "t_num_insert", "t_base_insert", "q_start", "q_end", "t_start", "t_end",
                                                  "n_blocks")] + [("block_off", "<u8")])  # k4_blitz_path
BLITZ_BLOCK_DTYPE = np.dtype([(n, "<u4") for n in ("len", "q_start", "t_start")])  # k4_blitz_block
PSL_HEADER = ("psLayout version 3", "")  # the two header lines of a PSL file that name no build


def psl_lines(index, names, queries, paths, blocks):
    """The PSL lines (CBlitz::ReportAsPSL, libkit4b/CBlitz.cpp:1925-2006; no newline) of the paths SfxIndex.blitz_paths / blitz returned
    for `queries`, whose names are `names`: 21 tab-separated columns, repMatches 0, qStart / qEnd flipped on '-', every block list
    ending in a comma.  Formatted on the host."""
    ents = {}
    out = []
    for p in paths:
        tid = int(p["targ_seq_id"])
        if tid not in ents:
            ents[tid] = index.entry(tid)
        qlen, plus = len(queries[int(p["query"])]), int(p["strand"]) == 0
        qs, qe = int(p["q_start"]), int(p["q_end"])
        b = blocks[int(p["block_off"]):int(p["block_off"]) + int(p["n_blocks"])]
        cols = [int(p["matches"]), int(p["mismatches"]), 0, int(p["n_count"]), int(p["q_num_insert"]), int(p["q_base_insert"]),
                int(p["t_num_insert"]), int(p["t_base_insert"]), "+" if plus else "-", names[int(p["query"])], qlen,
                qs if plus else qlen - (qe + 1), qe + 1 if plus else qlen - qs, ents[tid]["name"], ents[tid]["seq_len"], int(p["t_start"]),
                int(p["t_end"]) + 1, int(p["n_blocks"])]
        cols += ["".join("%d," % int(v) for v in b[f]) for f in ("len", "q_start", "t_start")]
        out.append("\t".join(str(c) for c in cols))
    return out


def build(verbose=False):
    """Compile libk4sfx.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(PKG_DIR, "csrc"), "-j4"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)


def lib():
    """The loaded C ABI; raises if the HIP extension has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise K4Error(-2, "%s is missing: run kit4b_amd.build() / make -C kit4b_amd/csrc" % LIB_PATH)
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 (soname libamdhip64.so.7).  Loading torch
    # first makes libk4sfx.so's NEEDED libamdhip64.so.7 resolve to that already-loaded copy; the other order leaves
    # two runtimes in the process and the second one finds no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u32, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64
    L.k4_open.argtypes = [C.c_char_p, i32, i32, C.POINTER(vp)]
    L.k4_open_async.argtypes = [C.c_char_p, i32, i32, C.POINTER(vp)]
    L.k4_open_wait.argtypes = [vp]
    L.k4_open_seconds.argtypes = [vp]
    L.k4_open_seconds.restype = C.c_double
    L.k4_open_host.argtypes = [u64, u32, vp, vp, u32, C.POINTER(Entry), C.c_char_p, i32, i32, C.POINTER(vp)]
    L.k4_open_device.argtypes = [u64, u32, vp, vp, i32, u32, C.POINTER(Entry), C.c_char_p, i32, i32, C.POINTER(vp)]
    L.k4_close.argtypes = [vp]
    L.k4_close.restype = None
    L.k4_last_error.argtypes = [vp]
    L.k4_last_error.restype = C.c_char_p
    L.k4_global_error.restype = C.c_char_p
    L.k4_info.argtypes = [vp, C.POINTER(Info)]
    L.k4_get_entry.argtypes = [vp, u32, C.POINTER(Entry)]
    L.k4_get_ident.argtypes = [vp, C.c_char_p]
    L.k4_set_max_iter.argtypes = [vp, i32]
    L.k4_set_fastq_quality.argtypes = [vp, i32]
    L.k4_get_seq.argtypes = [vp, u32, u32, vp, u32]
    L.k4_write_sfx.argtypes = [vp, C.c_char_p]
    L.k4_build_sa_device.argtypes = [u64, u32, vp, vp, i32]
    L.k4_reserve.argtypes = [vp, i64, C.c_int32, C.c_int32]
    L.k4_align_reads_batch.argtypes = [vp, C.POINTER(AlignParams), i64] + [vp] * 8
    L.k4_align_reads_batch_dev.argtypes = [vp, C.POINTER(AlignParams), i64, C.c_int32] + [vp] * 9
    L.k4_kalign_batch.argtypes = [vp, C.POINTER(KalignParams), i64] + [vp] * 5
    L.k4_best_matches_batch.argtypes = [vp, C.POINTER(AlignParams), i64] + [vp] * 6
    L.k4_best_matches_batch_dev.argtypes = [vp, C.POINTER(AlignParams), i64, C.c_int32] + [vp] * 7
    L.k4_kalign_batch_dev.argtypes = [vp, C.POINTER(KalignParams), i64, C.c_int32] + [vp] * 6
    L.k4_min_core_len.argtypes = [vp, i32, C.POINTER(C.c_int)]
    L.k4_get_counters.argtypes = [vp, C.POINTER(Counters)]
    L.k4_reset_counters.argtypes = [vp]
    L.k4_enable_kernel_timing.argtypes = [vp, i32]
    L.k4_get_kernel_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.k4_mate_rescue_batch.argtypes = [vp, i64, vp, vp, u64, vp, vp]
    L.k4_kalign_pe_batch.argtypes = [vp, C.POINTER(KalignParams), C.POINTER(PeParams), i64] + [vp] * 7
    L.k4_kalign_pe_batch_dev.argtypes = [vp, C.POINTER(KalignParams), C.POINTER(PeParams), i64, C.c_int32] + [vp] * 5
    L.k4_parse_fastx_dev.argtypes = [vp, vp, u64, u64, i32, i32, i64, vp, u64, vp, vp, vp, vp, C.POINTER(ParseInfo), vp]
    L.k4_prepare_reads_dev.argtypes = [vp, i32, i64, C.c_int32, C.c_int32, vp, vp, vp, vp, u64, vp, vp,
                                       C.POINTER(u64), C.POINTER(u64), C.POINTER(u32), vp]
    L.k4_assign_multi_dev.argtypes = [vp, i32, C.c_int32, i64, C.c_int32, vp, vp, C.POINTER(C.c_int64), vp]
    L.k4_select_hits_dev.argtypes = [vp, i64, C.c_int32, vp, vp, vp, vp]
    L.k4_format_sam_dev.argtypes = [vp, i32, i64, vp, vp, C.c_int32, vp, vp, vp, vp, C.POINTER(SamNames), C.POINTER(vp),
                                    C.POINTER(u64), C.POINTER(SamStats), vp, vp]
    L.k4_align_reads_ext_batch.argtypes = [vp, C.POINTER(AlignParams), i64] + [vp] * 9
    L.k4_align_reads_ext_batch_dev.argtypes = [vp, C.POINTER(AlignParams), i64, C.c_int32] + [vp] * 10
    L.k4_kalign_ext_batch.argtypes = [vp, C.POINTER(KalignParams), i64] + [vp] * 6
    L.k4_kalign_ext_batch_dev.argtypes = [vp, C.POINTER(KalignParams), i64, C.c_int32] + [vp] * 7
    L.k4_auto_trim_flanks_dev.argtypes = [vp, C.c_int32, i32, i64, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(C.c_int64), vp]
    L.k4_remove_orphan_juncts_dev.argtypes = [vp, u32, i64, C.c_int32, vp, vp, vp, C.POINTER(C.c_int64), vp]
    L.k4_reduce_pcr_dups_dev.argtypes = [vp, C.c_int32, i64, C.c_int32, vp, vp, C.POINTER(C.c_int64), vp]
    L.k4_pcr5_primer_correct_dev.argtypes = [vp, C.c_int32, C.c_int32, i32, i64, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(C.c_int64), vp]
    L.k4_align_stats_collect.argtypes = [vp, i32]
    L.k4_align_stats_dev.argtypes = [vp, i32, i64, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, C.POINTER(AlignStats), vp]
    L.k4_free_align_stats.argtypes = [C.POINTER(AlignStats)]
    L.k4_free_align_stats.restype = None
    L.k4_write_align_stats.argtypes = [vp, C.POINTER(AlignStats), u64, C.c_int32, C.c_int32, i32, C.c_char_p]
    L.k4_pipeline_align_stats.argtypes = [vp, C.POINTER(AlignStats)]
    L.k4_site_prefs_dev.argtypes = [vp, i32, i64, C.c_int32, C.c_int32, vp, vp, vp, C.POINTER(SitePrefs), vp]
    L.k4_free_site_prefs.argtypes = [C.POINTER(SitePrefs)]
    L.k4_free_site_prefs.restype = None
    L.k4_write_site_prefs.argtypes = [C.POINTER(SitePrefs), C.c_char_p]
    L.k4_pipeline_site_prefs.argtypes = [vp, C.c_int32, C.POINTER(SitePrefs)]
    L.k4_pe_insert_dist_dev.argtypes = [vp, i64, vp, C.POINTER(PeInsertDist), vp]
    L.k4_free_pe_insert_dist.argtypes = [C.POINTER(PeInsertDist)]
    L.k4_free_pe_insert_dist.restype = None
    L.k4_write_pe_insert_dist.argtypes = [vp, C.POINTER(PeInsertDist), u64, C.c_char_p]
    L.k4_pipeline_pe_insert_dist.argtypes = [vp, C.POINTER(PeInsertDist)]
    L.k4_pe_insert_bin_host.argtypes = [u32]
    L.k4_pe_insert_median_host.argtypes = [vp, u32, C.POINTER(u32)]
    L.k4_filter_loci_constraints_dev.argtypes = [vp, C.POINTER(LociConstraint), C.c_int32, i32, i64, C.c_int32, vp, vp, vp, vp, vp, vp, vp,
                                                 C.POINTER(C.c_int64), vp]
    L.k4_filter_chroms_dev.argtypes = [vp, vp, i32, i64, C.c_int32, vp, vp, C.POINTER(C.c_int64), vp]
    L.k4_filter_marked_prior.argtypes = [vp, C.POINTER(u64)]
    L.k4_set_priority_regions.argtypes = [vp, i64, vp, vp, vp]
    L.k4_filter_priority_regions_dev.argtypes = [vp, i32, i64, C.c_int32, vp, vp, vp, C.POINTER(C.c_int64), vp]
    L.k4_priority_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64)]
    L.k4_priority_select_dev.argtypes = [vp, i64, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.k4_load_loci_constraints.argtypes = [vp, C.c_char_p, C.POINTER(C.POINTER(LociConstraint)), C.POINTER(C.c_int32), C.c_char_p]
    L.k4_chrom_accept_mask.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_char_p), vp]
    L.k4_format_sam_ext_dev.argtypes = [vp, i32, i64, vp, vp, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(SamNames), C.POINTER(vp),
                                        C.POINTER(u64), C.POINTER(SamStats), vp, vp]
    L.k4_format_bam_dev.argtypes = [vp, i32, i64, vp, vp, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(SamNames), C.c_int32, C.POINTER(vp),
                                    C.POINTER(u64), C.POINTER(SamStats), vp, vp]
    L.k4_pipeline_format_bam.argtypes = [vp, C.c_int32, C.POINTER(SamStats), vp, C.POINTER(u64)]
    L.k4_pipeline_open.argtypes = [vp, C.POINTER(PipelineParams), C.POINTER(vp)]
    L.k4_pipeline_acquire.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u64)]
    L.k4_pipeline_submit.argtypes = [vp, i32, u64, i32]
    L.k4_pipeline_submit_host.argtypes = [vp, i32, vp, u64, i32]
    L.k4_pipeline_wait_aligned.argtypes = [vp, C.POINTER(PipelineView)]
    L.k4_pipeline_format.argtypes = [vp, C.POINTER(SamStats), vp, C.POINTER(u64)]
    L.k4_pipeline_next_sam.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.k4_pipeline_read_sam.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.k4_pipeline_close.argtypes = [vp]
    L.k4_pipeline_close.restype = None
    L.k4_free_device.argtypes = [vp]
    L.k4_free_device.restype = None
    L.k4_alloc_device.argtypes = [vp, u64, C.POINTER(vp)]
    L.k4_copy_to_device.argtypes = [vp, vp, vp, u64]
    L.k4_copy_to_host.argtypes = [vp, vp, vp, u64]
    L.k4_upload_pageable.argtypes = [i32, vp, vp, u64]
    L.k4_host_register.argtypes = [vp, u64]
    L.k4_host_unregister.argtypes = [vp]
    # (every argument list is declared: ctypes would otherwise pass a Python int -- a device address -- as a 32-bit C int)
    dbl, pvp, pu64 = C.c_double, C.POINTER(vp), C.POINTER(u64)
    fmt_head = [vp, i32, i64, vp, vp, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(SamNames)]  # ix .. names of the *_all / *_ext formatters
    L.k4_format_sam_all_dev.argtypes = fmt_head + [pvp, pu64, C.POINTER(SamStats), vp, vp]
    L.k4_format_bam_all_dev.argtypes = fmt_head + [C.c_int32, pvp, pu64, C.POINTER(SamStats), vp, vp]
    L.k4_pipeline_format_all.argtypes = [vp, C.POINTER(SamStats), vp, pu64]
    L.k4_pipeline_format_bam_all.argtypes = [vp, C.c_int32, C.POINTER(SamStats), vp, pu64]
    L.k4_pipeline_set_trims.argtypes = [vp, C.c_int32, C.c_int32]
    L.k4_pipeline_set_sampling.argtypes = [vp, C.c_int32]
    L.k4_unaligned_fasta_dev.argtypes = [vp, i32, i64, vp, vp, vp, vp, vp, C.POINTER(SamNames), C.c_int32, pvp, pu64, pu64, vp]
    L.k4_prepare_reads_trim_dev.argtypes = [vp, i32, i64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i64, vp, vp, vp, vp, u64,
                                            vp, vp, pu64, pu64, C.POINTER(u32), vp]
    L.k4_load_contaminants.argtypes = [vp, C.c_char_p, C.POINTER(C.POINTER(Contaminant)), C.POINTER(C.c_int32), C.c_char_p]
    L.k4_contam_match_host.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32]
    L.k4_contam_trims_dev.argtypes = [vp, vp, C.c_int32, i32, i64, C.c_int32, C.c_int32, C.c_int32, i64, vp, vp, vp, vp, vp, u64, vp, vp, pu64, vp]
    L.k4_prepare_reads_contam_dev.argtypes = [vp, i32, i64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i64, vp, vp, vp, vp, u64, vp, vp,
                                              vp, vp, pu64, pu64, C.POINTER(u32), pu64, vp]
    L.k4_pipeline_set_contaminants.argtypes = [vp, vp, C.c_int32]
    L.k4_pipeline_contam_totals.argtypes = [vp, pu64]
    snp_head = [vp, i32, i64, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_int32, dbl, dbl]  # ix, pe .. snp_nonref_pcnt
    L.k4_snp_csv_dev.argtypes = snp_head + [pvp, pu64, pu64, vp]
    L.k4_snp_vcf_dev.argtypes = snp_head + [pvp, pu64, pu64, vp]
    L.k4_snp_files_dev.argtypes = [vp, i32] + snp_head[1:] + [pvp, pu64, pu64, pvp, pu64, vp]
    L.k4_snp_run_dev.argtypes = [vp, i32] + snp_head[1:] + [vp, vp]
    L.k4_snp_run2_dev.argtypes = [vp, i32] + snp_head[1:] + [C.POINTER(SnpOpts), C.POINTER(SnpFiles2), vp]
    L.k4_marker_classify_host.argtypes = [vp, u64, u32, vp, C.c_int32, dbl, vp, vp]
    L.k4_free_host.argtypes = [vp]
    L.k4_free_host.restype = None
    L.k4_pba_run_dev.argtypes = [vp, i32, i64, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_char_p, C.c_char_p, C.POINTER(PbaFiles), vp]
    L.k4_pba_classify_host.argtypes = [vp, u64, u32, vp, vp, vp]
    L.k4_sfx_map.argtypes = [C.c_char_p, vp]
    L.k4_sfx_unmap.argtypes = [vp]
    L.k4_sfx_unmap.restype = None
    L.k4_set_raw_header.argtypes = [vp, vp]
    L.k4_set_description.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.k4_get_sfx_header.argtypes = [vp, vp]
    L.k4_abi_version.argtypes = []
    L.k4_global_error.argtypes = []
    L.k4_get_kernel_times_split.argtypes = [vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(C.c_int32)]
    L.k4_query_reserve.argtypes = [vp, C.POINTER(QueryParams), i64, u32]
    L.k4_locate_query_seqs_batch.argtypes = [vp, C.POINTER(QueryParams), i64, vp, vp, vp, vp, vp, u64]
    L.k4_locate_query_seqs_batch_dev.argtypes = [vp, C.POINTER(QueryParams), i64, u32, vp, vp, vp, vp, vp, u64, vp]
    L.k4_query_last_kernel_ms.argtypes = [vp]
    L.k4_query_last_kernel_ms.restype = dbl
    L.k4_blitz_paths_batch.argtypes = [vp, C.POINTER(BlitzParams), i64] + [vp] * 7 + [u64, vp, u64, vp]
    L.k4_blitz_paths_batch_dev.argtypes = [vp, C.POINTER(BlitzParams), i64] + [vp] * 7 + [u64, vp, u64, vp, vp]
    L.k4_blitz_last_kernel_ms.argtypes = [vp]
    L.k4_blitz_last_kernel_ms.restype = dbl
    L.k4_locate_sfx_hammings_batch.argtypes = [vp, C.POINTER(HammingParams), i64, vp, vp, vp, vp, vp, u64]
    L.k4_locate_sfx_hammings_batch_dev.argtypes = [vp, C.POINTER(HammingParams), i64, vp, vp, vp, vp, vp, u64, vp]
    L.k4_locate_hammings_batch.argtypes = [vp, C.POINTER(HammingParams), i64, vp, vp, vp, vp, vp, u64]
    L.k4_locate_hammings_batch_dev.argtypes = [vp, C.POINTER(HammingParams), i64, vp, vp, vp, vp, vp, u64, vp]
    L.k4_hamming_last_kernel_ms.argtypes = [vp]
    L.k4_hamming_last_kernel_ms.restype = dbl
    L.k4_kmer_cults_batch.argtypes = [vp, C.POINTER(CultsParams), i64, i64, C.POINTER(CultsOut), C.POINTER(CultsCaps), C.POINTER(CultsTotals)]
    L.k4_kmer_cults_batch_dev.argtypes = [vp, C.POINTER(CultsParams), i64, i64, C.POINTER(CultsOut), C.POINTER(CultsCaps), C.POINTER(CultsTotals), vp]
    L.k4_cults_last_kernel_ms.argtypes = [vp]
    L.k4_cults_last_kernel_ms.restype = dbl
    L.k4_exact_ranges_batch.argtypes = [vp, i64, vp, vp, vp, vp, vp]
    L.k4_exact_ranges_batch_dev.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
    L.k4_matches_other_chroms_batch.argtypes = [vp, C.c_int32, vp, C.c_int32, i64, vp, vp, vp, vp]
    L.k4_species_kmers_batch.argtypes = [vp, C.POINTER(KMarkersParams), C.c_int32, vp, vp, C.c_uint64, C.POINTER(KMarkersTotals)]
    L.k4_species_kmers_batch_dev.argtypes = [vp, C.POINTER(KMarkersParams), C.c_int32, vp, vp, C.c_uint64, C.POINTER(KMarkersTotals), vp]
    L.k4_kmarkers_last_kernel_ms.argtypes = [vp]
    L.k4_kmarkers_last_kernel_ms.restype = dbl
    L.k4_get_sfx_els.argtypes = [vp, u64, u64, vp]
    L.k4_all_near_matches_batch.argtypes = [vp, C.POINTER(NearParams), i64, vp, vp, vp, vp, vp, vp, vp, u64]
    L.k4_all_near_matches_batch_dev.argtypes = [vp, C.POINTER(NearParams), i64, vp, vp, vp, vp, vp, vp, vp, u64, vp]
    L.k4_zygosity_batch.argtypes = [vp, C.POINTER(ZygosityParams), C.c_int32, C.c_int32, vp, vp, vp, u64, C.POINTER(ZygosityTotals)]
    L.k4_zygosity_batch_dev.argtypes = [vp, C.POINTER(ZygosityParams), C.c_int32, C.c_int32, vp, vp, vp, u64, C.POINTER(ZygosityTotals), vp]
    L.k4_zygosity_last_kernel_ms.argtypes = [vp]
    L.k4_zygosity_last_kernel_ms.restype = dbl
    _lib = L
    return L


def _flatten(reads):
    if isinstance(reads, tuple):
        cat, offs, lens = reads
        return (np.ascontiguousarray(cat, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.uint64),
                np.ascontiguousarray(lens, dtype=np.uint32))
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(len(reads), dtype=np.uint64)
    if len(reads):
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        cat = np.ascontiguousarray(np.concatenate(reads).astype(np.uint8))
    else:
        cat = np.zeros(0, dtype=np.uint8)
    return cat, offs, lens


def gen_hash16(name):
    """CUtility::GenHash16 (libkit4b/Utility.cpp:402-420): the 16-bit hash of the lower-cased entry name"""
    if not name:
        return 0
    h = 19937
    for ch in name.lower():
        h = ((h ^ ch) * 3119) & 0xFFFFFFFF
        if h & 0x80000000:  # int arithmetic in the reference: the shift below is arithmetic
            h -= 1 << 32
        h ^= h >> 13
        h &= 0xFFFF
    return h or 19937


def make_entries(names, lens):
    """tsSfxEntry table for sequences concatenated with one EOS after each (CSfxArray::AddEntry, SfxArray.cpp:1735-1750)."""
    arr = (Entry * len(names))()
    ofs = 0
    for i, (nm, ln) in enumerate(zip(names, lens)):
        arr[i].entry_id = i + 1
        arr[i].fblock_id = 1
        arr[i].name = nm.encode() if isinstance(nm, str) else nm
        arr[i].name_hash = gen_hash16(arr[i].name)
        arr[i].seq_len = int(ln)
        arr[i].start_ofs = ofs
        arr[i].end_ofs = ofs + int(ln) - 1
        ofs += int(ln) + 1
    return arr


class SfxIndex:
    """HBM-resident index: the counterpart of an opened CSfxArray (libkit4b/SfxArray.h:524)."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)
        self._keep = []

    # -- construction -----------------------------------------------------------------------------------------
    @staticmethod
    def _check_open(rc, h):
        if rc != 0:
            raise K4Error(rc, lib().k4_global_error().decode())
        return SfxIndex(h.value)

    @classmethod
    def open(cls, path, device=0, kmer_k=0):
        h = C.c_void_p()
        return cls._check_open(lib().k4_open(path.encode(), device, kmer_k, C.byref(h)), h)

    @classmethod
    def from_host(cls, seq, sa_bytes, el_size, entries, dataset="syn", device=0, kmer_k=0):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        sa_bytes = np.ascontiguousarray(sa_bytes, dtype=np.uint8)
        h = C.c_void_p()
        rc = lib().k4_open_host(len(seq), el_size, seq.ctypes.data, sa_bytes.ctypes.data, len(entries), entries,
                                dataset.encode(), device, kmer_k, C.byref(h))
        return cls._check_open(rc, h)

    @classmethod
    def from_device(cls, concat_len, el_size, d_seq_ptr, d_sa_ptr, entries, dataset="syn", device=0, kmer_k=0,
                    adopt_sa=True, keep=()):
        h = C.c_void_p()
        rc = lib().k4_open_device(concat_len, el_size, d_seq_ptr, d_sa_ptr, 1 if adopt_sa else 0, len(entries),
                                  entries, dataset.encode(), device, kmer_k, C.byref(h))
        ix = cls._check_open(rc, h)
        ix._keep = list(keep)  # tensors whose storage the index adopted
        return ix

    def close(self):
        if self.h:
            lib().k4_close(self.h)
            self.h = C.c_void_p()

    def _ck(self, rc):
        if rc < 0:
            raise K4Error(rc, lib().k4_last_error(self.h).decode())
        return rc

    # -- accessors ----------------------------------------------------------------------------------------------
    def info(self):
        o = Info()
        self._ck(lib().k4_info(self.h, C.byref(o)))
        return {f[0]: (getattr(o, f[0]).decode() if f[0] == "dataset" else getattr(o, f[0])) for f in Info._fields_}

    def entry(self, entry_id):
        e = Entry()
        self._ck(lib().k4_get_entry(self.h, entry_id, C.byref(e)))
        return dict(entry_id=e.entry_id, name=e.name.decode(), seq_len=e.seq_len, start_ofs=e.start_ofs,
                    end_ofs=e.end_ofs)

    def get_ident(self, name):
        return lib().k4_get_ident(self.h, name.encode())

    def set_max_iter(self, it):
        return lib().k4_set_max_iter(self.h, it)

    def set_fastq_quality(self, method):
        """kalign -g: 0 Sanger, 1 Illumina 1.3+, 2 Solexa, 3 ignore the quality lines (default)"""
        self._ck(lib().k4_set_fastq_quality(self.h, method))

    def get_seq(self, entry_id, loci, length):
        out = np.zeros(length, dtype=np.uint8)
        n = lib().k4_get_seq(self.h, entry_id, loci, out.ctypes.data, length)
        return out[:n]

    def write_sfx(self, path):
        self._ck(lib().k4_write_sfx(self.h, path.encode()))

    def min_core_len(self, pmode=0):
        s = C.c_int(0)
        m = self._ck(lib().k4_min_core_len(self.h, pmode, C.byref(s)))
        return m, s.value

    def counters(self):
        c = Counters()
        self._ck(lib().k4_get_counters(self.h, C.byref(c)))
        return {f[0]: getattr(c, f[0]) for f in Counters._fields_}

    def reset_counters(self):
        self._ck(lib().k4_reset_counters(self.h))

    def enable_kernel_timing(self, on=True):
        self._ck(lib().k4_enable_kernel_timing(self.h, 1 if on else 0))

    def kernel_times(self):
        """(summed k4k_align_step milliseconds, launches) since the last call; synchronises."""
        ms, n = C.c_double(0), C.c_int32(0)
        self._ck(lib().k4_get_kernel_times(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_times_split(self):
        """(k4k_align_step ms, k4k_align_slow ms, batches) since the last call; synchronises."""
        ms, g, n = C.c_double(0), C.c_double(0), C.c_int32(0)
        self._ck(lib().k4_get_kernel_times_split(self.h, C.byref(ms), C.byref(g), C.byref(n)))
        return ms.value, g.value, n.value

    def reserve(self, max_reads, max_read_len, max_hits):
        self._ck(lib().k4_reserve(self.h, max_reads, max_read_len, max_hits))

    # -- the hot path (host buffers) ----------------------------------------------------------------------------
    def align_reads_batch(self, reads, tot_mm, core_len, core_delta, max_slides, min_core_len=0, mm_delta=1,
                          strand=STRAND_BOTH, max_hits=1):
        """CSfxArray::AlignReads (libkit4b/SfxArray.h:614) for a batch of fresh reads."""
        cat, offs, lens = _flatten(reads)
        n = len(lens)
        p = AlignParams(tot_mm, core_len, core_delta, max_slides, min_core_len, mm_delta, strand, max_hits)
        rslt = np.zeros(n, np.int32); inst = np.zeros(n, np.int32); low = np.zeros(n, np.int32)
        nxt = np.zeros(n, np.int32)
        hits = np.zeros((n, max_hits), dtype=HIT_DTYPE)
        self._ck(lib().k4_align_reads_batch(self.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data,
                                            lens.ctypes.data, rslt.ctypes.data, inst.ctypes.data, low.ctypes.data,
                                            nxt.ctypes.data, hits.ctypes.data))
        return dict(rslt=rslt, inst=inst, low=low, nxt=nxt, hits=hits)

    def align_reads_ext_batch(self, reads, tot_mm, core_len, core_delta, max_slides, min_core_len=0, mm_delta=1,
                              strand=STRAND_BOTH, max_hits=1, min_chimeric_len=0, micro_indel_len=0, max_splice_junct_len=0):
        """CSfxArray::AlignReads with MinChimericLen / microInDelLen / MaxSpliceJunctLen (SfxArray.cpp:7894-7930)."""
        cat, offs, lens = _flatten(reads)
        n = len(lens)
        p = AlignParams(tot_mm, core_len, core_delta, max_slides, min_core_len, mm_delta, strand, max_hits,
                        min_chimeric_len, micro_indel_len, max_splice_junct_len)
        rslt = np.zeros(n, np.int32); inst = np.zeros(n, np.int32); low = np.zeros(n, np.int32)
        nxt = np.zeros(n, np.int32)
        hits = np.zeros((n, max_hits), dtype=HIT_DTYPE)
        seg2 = np.zeros(n, dtype=SEG2_DTYPE)
        self._ck(lib().k4_align_reads_ext_batch(self.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                                rslt.ctypes.data, inst.ctypes.data, low.ctypes.data, nxt.ctypes.data,
                                                hits.ctypes.data, seg2.ctypes.data))
        return dict(rslt=rslt, inst=inst, low=low, nxt=nxt, hits=hits, seg2=seg2)

    def kalign_ext_batch(self, reads, max_subs=5, min_edit_dist=1, max_ns=1, pmode=0, strand=STRAND_BOTH, max_ml=1,
                         pe_mode=0, min_core_len=0, max_num_slides=0, min_chimeric_len=0, micro_indel_len=0,
                         max_splice_junct_len=0):
        """CKAligner::AlignRead with -c / -a / -A."""
        cat, offs, lens = _flatten(reads)
        n = len(lens)
        p = KalignParams(max_subs, min_edit_dist, max_ns, pmode, strand, max_ml, pe_mode, min_core_len, max_num_slides,
                         min_chimeric_len, micro_indel_len, max_splice_junct_len)
        out = np.zeros(n, dtype=RESULT_DTYPE)
        hits = np.zeros((n, max(1, max_ml)), dtype=HIT_DTYPE)
        seg2 = np.zeros(n, dtype=SEG2_DTYPE)
        self._ck(lib().k4_kalign_ext_batch(self.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                           out.ctypes.data, hits.ctypes.data, seg2.ctypes.data))
        return dict(out=out, hits=hits, seg2=seg2)

    def best_matches_batch(self, reads, tot_mm, core_len, core_delta, max_core_slides, strand=STRAND_BOTH, max_hits=5):
        """CSfxArray::LocateBestMatches over a batch: rslt (the call's return value), inst, hits[n, max_hits]."""
        cat, offs, lens = _flatten(reads)
        n = len(lens)
        p = AlignParams(tot_mm, core_len, core_delta, max_core_slides, 0, 1, strand, max_hits)
        rslt = np.zeros(n, dtype=np.int32)
        inst = np.zeros(n, dtype=np.int32)
        hits = np.zeros((n, max_hits), dtype=HIT_DTYPE)
        self._ck(lib().k4_best_matches_batch(self.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                             rslt.ctypes.data, inst.ctypes.data, hits.ctypes.data))
        return dict(rslt=rslt, inst=inst, hits=hits)

    def locate_query_seqs(self, queries, core_len=20, core_delta=10, strand=STRAND_BOTH, max_hits=1000, max_iter=100, match_pts=1,
                          mismatch_pts=3, nodes_cap=None):
        """CSfxArray::LocateQuerySeqs (libkit4b/SfxArray.h:779) for a batch of query sequences: per query a QUERY_NODE_DTYPE array of
        its nodes in the reference's order.  nodes_cap: capacity of the output (default: grown until everything fits); when it is
        given and too small the K4Error (code -95) carries the capacity needed as `.needed`."""
        cat, offs, lens = _flatten(queries)
        n = len(lens)
        p = QueryParams(core_len, core_delta, strand, max_hits, max_iter, match_pts, mismatch_pts)
        node_offs = np.zeros(n + 1, dtype=np.uint64)
        cap = max(1, 4 * n) if nodes_cap is None else int(nodes_cap)
        while True:
            nodes = np.zeros(max(cap, 1), dtype=QUERY_NODE_DTYPE)
            rc = lib().k4_locate_query_seqs_batch(self.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                                  node_offs.ctypes.data, nodes.ctypes.data, cap)
            if rc == -95 and int(node_offs[n]) > cap:
                if nodes_cap is None:
                    cap = int(node_offs[n])
                    continue
                e = K4Error(rc, lib().k4_last_error(self.h).decode())
                e.needed = int(node_offs[n])
                raise e
            self._ck(rc)
            return [nodes[int(node_offs[i]):int(node_offs[i + 1])].copy() for i in range(n)]

    def query_kernel_ms(self):
        """device milliseconds of the last locate_query_seqs batch (the locate kernel, rocPRIM's scan of the counts, the gather kernel);
        0 for a batch of no queries"""
        return lib().k4_query_last_kernel_ms(self.h)

    def blitz_paths(self, queries, node_offs, nodes, match_pts=1, mismatch_pts=2, gap_open=5, min_path_score=0, query_len_aligned_pct=75,
                    max_paths=1, strand=STRAND_BOTH, paths_cap=None, blocks_cap=None):
        """CBlitz's path stage (libkit4b/CBlitz.cpp) over the nodes locate_query_seqs found: (path_offs, paths, blocks) as uint64 /
        BLITZ_PATH_DTYPE / BLITZ_BLOCK_DTYPE arrays; the paths of query i are paths[path_offs[i]:path_offs[i + 1]] in the reference's
        report order.  nodes: one QUERY_NODE_DTYPE array behind node_offs, or the per-query list locate_query_seqs returns (node_offs
        None).  A capacity that is given and too small raises K4Error -95 with `.needed` = (paths, blocks)."""
        cat, offs, lens = _flatten(queries)
        n = len(lens)
        if node_offs is None:
            node_offs = np.concatenate([[0], np.cumsum([len(a) for a in nodes])]).astype(np.uint64)
            nodes = np.concatenate(list(nodes)) if n else np.zeros(0, QUERY_NODE_DTYPE)
        node_offs = np.ascontiguousarray(node_offs, dtype=np.uint64)
        nodes = np.ascontiguousarray(nodes, dtype=QUERY_NODE_DTYPE)
        p = BlitzParams(match_pts, mismatch_pts, gap_open, min_path_score, query_len_aligned_pct, max_paths, strand)
        caps = [n * max(1, max_paths) if paths_cap is None else int(paths_cap), len(nodes) if blocks_cap is None else int(blocks_cap)]
        path_offs = np.zeros(n + 1, dtype=np.uint64)
        paths = np.zeros(max(caps[0], 1), dtype=BLITZ_PATH_DTYPE)
        blocks = np.zeros(max(caps[1], 1), dtype=BLITZ_BLOCK_DTYPE)
        needed = np.zeros(2, dtype=np.uint64)
        rc = lib().k4_blitz_paths_batch(self.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data, node_offs.ctypes.data,
                                        nodes.ctypes.data, path_offs.ctypes.data, paths.ctypes.data, caps[0], blocks.ctypes.data, caps[1],
                                        needed.ctypes.data)
        if rc == -95:
            e = K4Error(rc, lib().k4_last_error(self.h).decode())
            e.needed = (int(needed[0]), int(needed[1]))
            raise e
        self._ck(rc)
        return path_offs, paths[:int(needed[0])].copy(), blocks[:int(needed[1])].copy()

    def blitz(self, queries, core_len=20, core_delta=10, max_hits=200000, max_iter=100, match_pts=1, mismatch_pts=2, gap_open=5,
              min_path_score=0, query_len_aligned_pct=75, max_paths=1, strand=STRAND_BOTH):
        """`ngskit4b blitz` for a batch of queries, both stages on the device with the nodes staying there in between: LocateQuerySeqs
        (k4_locate_query_seqs_batch_dev), then the path stage (k4_blitz_paths_batch_dev).  Returns (path_offs, paths, blocks) as
        blitz_paths does; psl_lines() makes the PSL text.  locate_ms / paths_ms of the call are left in self.blitz_ms."""
        L = lib()
        cat, offs, lens = _flatten(queries)
        n = len(lens)
        max_len = int(lens.max()) if n else 0
        qp = QueryParams(core_len, core_delta, strand, max_hits, max_iter, match_pts, mismatch_pts)
        bp = BlitzParams(match_pts, mismatch_pts, gap_open, min_path_score, query_len_aligned_pct, max_paths, strand)
        held = []

        def dev(nbytes, src=None):
            d = C.c_void_p()
            self._ck(L.k4_alloc_device(self.h, max(int(nbytes), 16), C.byref(d)))
            held.append(d)
            if src is not None and src.nbytes:
                self._ck(L.k4_copy_to_device(self.h, d, src.ctypes.data, src.nbytes))
            return d

        try:
            d_seqs, d_offs, d_lens = dev(cat.nbytes + 16, cat), dev(offs.nbytes, offs), dev(lens.nbytes, lens)
            d_node_offs = dev((n + 1) * 8)
            cap = max(64, 8 * n)
            node_offs = np.zeros(n + 1, dtype=np.uint64)
            while True:
                d_nodes = dev(cap * QUERY_NODE_DTYPE.itemsize)
                rc = L.k4_locate_query_seqs_batch_dev(self.h, C.byref(qp), n, max_len, d_seqs, d_offs, d_lens, d_node_offs, d_nodes, cap, None)
                self._ck(L.k4_copy_to_host(self.h, node_offs.ctypes.data, d_node_offs, node_offs.nbytes))
                if rc == -95 and int(node_offs[n]) > cap:
                    cap = int(node_offs[n])
                    continue
                self._ck(rc)
                break
            locate_ms = L.k4_query_last_kernel_ms(self.h)
            total = int(node_offs[n])
            caps = [max(1, n * max_paths), max(1, total)]
            d_path_offs, d_paths, d_blocks = dev((n + 1) * 8), dev(caps[0] * BLITZ_PATH_DTYPE.itemsize), dev(caps[1] * BLITZ_BLOCK_DTYPE.itemsize)
            needed = np.zeros(2, dtype=np.uint64)
            self._ck(L.k4_blitz_paths_batch_dev(self.h, C.byref(bp), n, d_seqs, d_offs, d_lens, d_node_offs, d_nodes, d_path_offs, d_paths, caps[0],
                                                d_blocks, caps[1], needed.ctypes.data, None))
            self.blitz_ms = (locate_ms, L.k4_blitz_last_kernel_ms(self.h))
            path_offs = np.zeros(n + 1, dtype=np.uint64)
            paths = np.zeros(int(needed[0]), dtype=BLITZ_PATH_DTYPE)
            blocks = np.zeros(int(needed[1]), dtype=BLITZ_BLOCK_DTYPE)
            self._ck(L.k4_copy_to_host(self.h, path_offs.ctypes.data, d_path_offs, path_offs.nbytes))
            if len(paths):
                self._ck(L.k4_copy_to_host(self.h, paths.ctypes.data, d_paths, paths.nbytes))
            if len(blocks):
                self._ck(L.k4_copy_to_host(self.h, blocks.ctypes.data, d_blocks, blocks.nbytes))
            return path_offs, paths, blocks
        finally:
            for d in held:
                L.k4_free_device(d)

    def sfx_hammings(self, spans, kmer_len, rhamm, min_core_depth, max_core_depth, both_strands=False, sample_nth=1, intra_inter_both=0,
                     out=None, out_offs=None):
        """CSfxArray::LocateSfxHammings (libkit4b/SfxArray.cpp:4107) for a batch of spans [(entry_id, entry_loci, span_len)]: a list
        of uint8 arrays of span_len bytes, 0xFF where the reference writes nothing.  With out (uint8) and out_offs the bytes go into
        that array instead, which is returned."""
        sp = np.array(spans, dtype=np.int64).reshape(-1, 3)
        n = len(sp)
        ids, locis, lens = (np.ascontiguousarray(sp[:, k].astype(np.uint32)) for k in range(3))
        own = out is None
        if own:
            out_offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64) if n else np.zeros(0, np.uint64)
            out = np.full(max(int(lens.sum()), 1), 0xFF, dtype=np.uint8)
        out_offs = np.ascontiguousarray(out_offs, dtype=np.uint64)
        p = HammingParams(rhamm, kmer_len, sample_nth, 1 if both_strands else 0, min_core_depth, max_core_depth, intra_inter_both)
        self._ck(lib().k4_locate_sfx_hammings_batch(self.h, C.byref(p), n, ids.ctypes.data, locis.ctypes.data, lens.ctypes.data,
                                                    out_offs.ctypes.data, out.ctypes.data, len(out)))
        return [out[int(o):int(o) + int(l)].copy() for o, l in zip(out_offs, lens)] if own else out

    def hammings(self, seqs, kmer_len, rhamm, min_core_depth, max_core_depth, both_strands=False, sample_nth=1, intra_inter_both=0):
        """CSfxArray::LocateHammings (libkit4b/SfxArray.cpp:4227) with SeqEntry 0 for a batch of sequences (codes 0..4): per sequence
        a uint8 array of its length, 0xFF where the reference writes nothing."""
        cat, offs, lens = _flatten(seqs)
        n = len(lens)
        out = np.full(max(len(cat), 1), 0xFF, dtype=np.uint8)
        cat = np.concatenate([cat, np.zeros(16, np.uint8)])
        p = HammingParams(rhamm, kmer_len, sample_nth, 1 if both_strands else 0, min_core_depth, max_core_depth, intra_inter_both)
        self._ck(lib().k4_locate_hammings_batch(self.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data, offs.ctypes.data,
                                                out.ctypes.data, len(out)))
        return [out[int(o):int(o) + int(l)].copy() for o, l in zip(offs, lens)]

    def restricted_hammings(self, kmer_len, rhamm, sensitivity=0, both_strands=False, sample_nth=1, intra_inter_both=0):
        """`ngskit4b hammings -m0` over the index itself (GenRestrictedHammings, ngskit4b/hammings.cpp:2313-2405): one byte per base of
        every entry, 0xFF where no Hamming was generated.  sensitivity 0 default, 1 more, 2 ultra, 3 less (the reference's -s); the
        spans are cut as its worker threads cut them (hamming_spans), which decides the sampled loci when sample_nth > 1.
        hammings_csv() makes the report."""
        depths = {0: HAMMING_DEPTHS[1], 1: HAMMING_DEPTHS[2], 2: HAMMING_DEPTHS[3], 3: HAMMING_DEPTHS[0]}[sensitivity]
        n = self.info()["n_entries"]
        lens = [self.entry(e)["seq_len"] for e in range(1, n + 1)]
        out = np.full(max(sum(lens), 1), 0xFF, dtype=np.uint8)
        ids, locis, sl, offs = hamming_spans(lens, kmer_len)
        if len(ids):
            self.sfx_hammings(np.stack([ids, locis, sl], axis=1), kmer_len, rhamm, depths[0], depths[1], both_strands, sample_nth,
                              intra_inter_both, out=out, out_offs=offs)
        return out[:sum(lens)]

    def hamming_kernel_ms(self):
        """device milliseconds of the last Hammings batch"""
        return lib().k4_hamming_last_kernel_ms(self.h)

    def sfx_els(self, first, n):
        """n suffix array elements from `first` (SfxOfsToLoci)"""
        out = np.zeros(n, dtype=np.uint64)
        self._ck(lib().k4_get_sfx_els(self.h, first, n, out.ctypes.data))
        return out

    def kmer_cults(self, prefix_len, suffix_len=0, min_cultivars=0, sense_only=False, start_sfx_idx=0, end_sfx_idx=0, max_window=0,
                   max_homozygotic=0, max_kmers=1 << 16, max_dist=None):
        """CSfxArray::GenKMerCultsCnts (libkit4b/SfxArray.cpp:2804) over suffix array elements start_sfx_idx .. end_sfx_idx: a dict
        of n_located (the reference's return value) and, for the K-mers it would hand to its callback, in its order, `kmers`
        (CULT_KMER_DTYPE), `bases` (n x K codes) and `dist` (CULT_DIST_DTYPE; K-mer i owns dist[dist_ofs : dist_ofs + num_cultivars]).
        The resumable call is repeated with room for max_kmers K-mers and max_dist counts until the range is done."""
        n_entries = self.info()["n_entries"]
        klen = prefix_len + suffix_len
        p = CultsParams(prefix_len, suffix_len, min_cultivars, 1 if sense_only else 0, max_window, max_homozygotic)
        max_dist = max(n_entries, 8 * max_kmers) if max_dist is None else max_dist
        kmers = np.zeros(max_kmers, dtype=CULT_KMER_DTYPE)
        bases = np.zeros((max_kmers, max(klen, 1)), dtype=np.uint8)
        dist = np.zeros(max_dist, dtype=CULT_DIST_DTYPE)
        out = CultsOut(kmers.ctypes.data, bases.ctypes.data, dist.ctypes.data)
        caps, tot = CultsCaps(max_kmers, max_dist), CultsTotals()
        parts, located, cur, n_dist = [], 0, start_sfx_idx, 0
        while True:
            self._ck(lib().k4_kmer_cults_batch(self.h, C.byref(p), cur, end_sfx_idx, C.byref(out), C.byref(caps), C.byref(tot)))
            k = kmers[:tot.n_kmers].copy()
            k["dist_ofs"] += n_dist
            parts.append((k, bases[:tot.n_kmers].copy(), dist[:tot.n_dist].copy()))
            located += tot.n_located
            n_dist += tot.n_dist
            if tot.done:
                break
            cur = tot.next_sfx_idx
        return dict(n_located=located, kmers=np.concatenate([q[0] for q in parts]), bases=np.concatenate([q[1] for q in parts]),
                    dist=np.concatenate([q[2] for q in parts]))

    def kmer_cult_thread_range(self, kmer_len, thread_inst, num_threads, start_sfx_idx):
        """CSfxArray::GenKMerCultThreadRange (libkit4b/SfxArray.cpp:2733): (rc, end_sfx_idx), on the host from a few elements and bases"""
        inf = self.info()
        if getattr(self, "_ent_starts", None) is None:  # (the table does not change while the index is open)
            ents = [self.entry(i + 1) for i in range(inf["n_entries"])]
            self._ent_starts, self._ents = [e["start_ofs"] for e in ents], ents
        block = {}

        def sa_at(i):  # elements come down 256 at a time: the walk looks at neighbours
            b0 = i - i % 256
            if b0 not in block:
                block.clear()
                block[b0] = self.sfx_els(b0, min(256, inf["concat_len"] - b0))
            return int(block[b0][i - b0])

        def bases_at(psn, n):
            e = self._ents[max(bisect.bisect_right(self._ent_starts, psn) - 1, 0)]
            return self.get_seq(e["entry_id"], psn - e["start_ofs"], n) if e["start_ofs"] <= psn < e["start_ofs"] + e["seq_len"] else []

        return kmer_cult_thread_range(inf["concat_len"], sa_at, bases_at, kmer_len, thread_inst, num_threads, start_sfx_idx)

    def cults_kernel_ms(self):
        """device milliseconds of the last kmer_cults call's launches"""
        return lib().k4_cults_last_kernel_ms(self.h)

    def exact_ranges(self, probes):
        """CSfxArray::IterateExacts walked to its end for a batch of probes (codes): (firsts uint64, counts uint32) -- the suffix
        index of a probe's first exact match and how many suffixes match; 0, 0 without one.  firsts + 1 is IterateExacts' return."""
        cat, offs, lens = _flatten(probes)
        n = len(lens)
        firsts, counts = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        cat = np.concatenate([cat, np.zeros(16, np.uint8)])
        self._ck(lib().k4_exact_ranges_batch(self.h, n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data, firsts.ctypes.data, counts.ctypes.data))
        return firsts, counts

    def matches_other_chroms(self, probe_ids, max_tot_mm, probes):
        """CSfxArray::MatchesOtherChroms (libkit4b/SfxArray.cpp:5094-5235) for a batch of probes against the entries whose ids are
        not in probe_ids (an id or a list): an int32 array of the reference's 1 / 0"""
        ids = np.ascontiguousarray(np.atleast_1d(probe_ids), dtype=np.uint32)
        cat, offs, lens = _flatten(probes)
        n = len(lens)
        out = np.zeros(n, dtype=np.int32)
        cat = np.concatenate([cat, np.zeros(16, np.uint8)])
        self._ck(lib().k4_matches_other_chroms_batch(self.h, len(ids), ids.ctypes.data, max_tot_mm, n, cat.ctypes.data, offs.ctypes.data,
                                                     lens.ctypes.data, out.ctypes.data))
        return out

    def species_kmers(self, target_ids, kmer_len, min_hamming=1, mode=0, prefix_len=0, min_with_prefix=0):
        """CLocKMers::LocateSpeciesUniqueKMers (ngskit4b/LocKMers.cpp:1085-1232) as one thread runs it over the targets in the order
        given: (status bytes, one per start locus of every target, KMER_NOT_KMER .. KMER_ACCEPTED; the front end's tallies as a dict)"""
        ids = np.ascontiguousarray(target_ids, dtype=np.uint32)
        total = 0
        for t in ids.tolist():
            e = Entry()
            if lib().k4_get_entry(self.h, t, C.byref(e)) == 0 and e.entry_id == t:
                total += e.seq_len
        status = np.zeros(max(total, 1), dtype=np.uint8)
        p = KMarkersParams(kmer_len, min_hamming, mode, prefix_len, min_with_prefix, 0)
        tot = KMarkersTotals()
        self._ck(lib().k4_species_kmers_batch(self.h, C.byref(p), len(ids), ids.ctypes.data, status.ctypes.data, len(status), C.byref(tot)))
        return status[:total], {f[0]: int(getattr(tot, f[0])) for f in KMarkersTotals._fields_}

    def kmarkers_kernel_ms(self):
        """device milliseconds of the last exact_ranges / matches_other_chroms / species_kmers call's launches"""
        return lib().k4_kmarkers_last_kernel_ms(self.h)

    def all_near_matches(self, probes, probe_entries, probe_ofs, max_tot_mm, core_len, core_delta, max_core_slides, max_matches=0,
                         cur_max_iter=0, n_ident_nodes=1024000, counts=True):
        """CSfxArray::LocateAllNearMatches (libkit4b/SfxArray.cpp:4820-5091) for a batch of probes (codes) that came from the entries
        with ids probe_entries at probe_ofs: (rslts int32: -1 or the matches in other entries; counts uint32 n x n_entries by entry
        id - 1, or None)"""
        cat, offs, lens = _flatten(probes)
        n = len(lens)
        ents = np.ascontiguousarray(probe_entries, dtype=np.uint32)
        pofs = np.ascontiguousarray(probe_ofs, dtype=np.uint32)
        if len(ents) != n or len(pofs) != n:
            raise ValueError("one probe entry and one offset per probe")
        n_ent = self.info()["n_entries"]
        rslts = np.zeros(n, dtype=np.int32)
        cnt = np.zeros((n, n_ent), dtype=np.uint32) if counts else None
        cat = np.concatenate([cat, np.zeros(16, np.uint8)])
        p = NearParams(max_tot_mm, core_len, core_delta, max_core_slides, max_matches, cur_max_iter, n_ident_nodes, 0)
        self._ck(lib().k4_all_near_matches_batch(self.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data, ents.ctypes.data,
                                                 pofs.ctypes.data, rslts.ctypes.data, cnt.ctypes.data if counts else None, n * n_ent))
        return rslts, cnt

    def zygosity(self, subseq_len=25, max_subs=2, max_ns=1, max_matches=5000, mode=0, src_first=1, src_count=None, status=False):
        """`genzygosity`'s scan (genzygosity/genzygosity.cpp:1122-1236) over the source entries src_first .. (ordinals, all by default):
        (matrix uint32 src_count x n_entries, subseqs uint32, totals dict[, status bytes: one ZYG_* per start locus of the sources])"""
        n_ent = self.info()["n_entries"]
        if src_count is None:
            src_count = max(n_ent - src_first + 1, 0)
        rows = max(src_count, 0)
        loci = sum(self.entry(src_first + r)["seq_len"] for r in range(rows) if 1 <= src_first + r <= n_ent)
        matrix, subseqs = np.zeros((rows, n_ent), dtype=np.uint32), np.zeros(rows, dtype=np.uint32)
        st = np.zeros(max(loci, 1), dtype=np.uint8) if status else None
        p = ZygosityParams(subseq_len, max_subs, max_ns, max_matches, mode, 0)
        tot = ZygosityTotals()
        m_arg = matrix if matrix.size else np.zeros(1, np.uint32)
        s_arg = subseqs if subseqs.size else np.zeros(1, np.uint32)
        self._ck(lib().k4_zygosity_batch(self.h, C.byref(p), src_first, src_count, m_arg.ctypes.data, s_arg.ctypes.data,
                                         st.ctypes.data if status else None, len(st) if status else 0, C.byref(tot)))
        out = (matrix, subseqs, {f[0]: int(getattr(tot, f[0])) for f in ZygosityTotals._fields_})
        return out + (st[:loci],) if status else out

    def zygosity_kernel_ms(self):
        """device milliseconds of the last all_near_matches / zygosity call's launches"""
        return lib().k4_zygosity_last_kernel_ms(self.h)

    def kalign_batch(self, reads, max_subs=5, min_edit_dist=1, max_ns=1, pmode=0, strand=STRAND_BOTH, max_ml=1,
                     pe_mode=0, min_core_len=0, max_num_slides=0):
        """CKAligner::AlignRead (ngskit4b/KAligner.cpp:9583) for a batch."""
        cat, offs, lens = _flatten(reads)
        n = len(lens)
        p = KalignParams(max_subs, min_edit_dist, max_ns, pmode, strand, max_ml, pe_mode, min_core_len,
                         max_num_slides)
        out = np.zeros(n, dtype=RESULT_DTYPE)
        hits = np.zeros((n, max(1, max_ml)), dtype=HIT_DTYPE)
        self._ck(lib().k4_kalign_batch(self.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                       out.ctypes.data, hits.ctypes.data))
        return dict(out=out, hits=hits)

    def kalign_pe_batch(self, reads1, reads2, pe_mode=2, pair_min_len=100, pair_max_len=1000, pair_strand=False,
                        max_subs=5, min_edit_dist=1, max_ns=1, pmode=0, strand=STRAND_BOTH, min_core_len=0,
                        max_num_slides=0, min_chimeric_len=0, max_ml=10):
        """CKAligner's PE flow (ProcCoredApprox + ProcessPairedEnds); out[2i] = PE1, out[2i+1] = PE2.  min_chimeric_len
        (kalign -c): chimeric trimming of both ends and of rescued mates; the trims come back in hit.ext.  max_ml: the SE
        pass keeps max(max_ml, 10) hit slots per end (cMaxMLPEmatches)."""
        c1, o1, l1 = _flatten(reads1)
        c2, o2, l2 = _flatten(reads2)
        assert len(l1) == len(l2)
        kp = KalignParams(max_subs, min_edit_dist, max_ns, pmode, strand, max_ml, 1, min_core_len, max_num_slides, min_chimeric_len, 0, 0)
        pe = PeParams(pe_mode, pair_min_len, pair_max_len, 1 if pair_strand else 0)
        out = np.zeros(2 * len(l1), dtype=PE_READ_DTYPE)
        self._ck(lib().k4_kalign_pe_batch(self.h, C.byref(kp), C.byref(pe), len(l1), c1.ctypes.data, o1.ctypes.data,
                                          l1.ctypes.data, c2.ctypes.data, o2.ctypes.data, l2.ctypes.data,
                                          out.ctypes.data))
        return out

    # -- read ingest and SAM emit on the device ----------------------------------------------------------------------
    def parse_fastx(self, text, fmt=0, chunk_bytes=None, device=None):
        """FASTA / FASTQ bytes -> dict of device tensors (reads u8, offs i64, lens i32, name_off i64, name_len i32) plus
        the text tensor they point into.  chunk_bytes < len(text) exercises the chunked protocol."""
        import torch

        dev = torch.device("cuda", self.info()["device"]) if device is None else device
        raw = np.frombuffer(bytes(text), dtype=np.uint8)
        T = len(raw)
        d_text = torch.from_numpy(np.concatenate([raw, np.zeros(16, np.uint8)])).to(dev)
        cap = int((raw == 10).sum()) // 2 + 4
        d_reads = torch.zeros(T + 32, dtype=torch.uint8, device=dev)
        d_offs = torch.zeros(cap, dtype=torch.int64, device=dev)
        d_lens = torch.zeros(cap, dtype=torch.int32, device=dev)
        d_noff = torch.zeros(cap, dtype=torch.int64, device=dev)
        d_nlen = torch.zeros(cap, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        pos, n, bases, max_len = 0, 0, 0, 0
        chunk = T if not chunk_bytes else chunk_bytes
        while pos < T:
            ln = min(chunk, T - pos)
            final = 1 if pos + ln == T else 0
            info = ParseInfo()
            self._ck(lib().k4_parse_fastx_dev(self.h, d_text.data_ptr() + pos, ln, pos, final, fmt, cap - n, d_reads.data_ptr(),
                                              bases, d_offs.data_ptr() + 8 * n, d_lens.data_ptr() + 4 * n,
                                              d_noff.data_ptr() + 8 * n, d_nlen.data_ptr() + 4 * n, C.byref(info), st))
            fmt = info.format or fmt
            if info.consumed == 0:
                if final:
                    break
                chunk *= 2  # a record longer than the chunk
                continue
            n += info.n_records
            bases += info.n_bases
            max_len = max(max_len, info.max_len)
            pos += info.consumed
        return {"n": n, "n_bases": bases, "max_len": max_len, "format": fmt, "text": d_text, "reads": d_reads,
                "offs": d_offs[:n], "lens": d_lens[:n], "name_off": d_noff[:n], "name_len": d_nlen[:n]}

    def prepare_reads(self, p1, p2=None, min_len=50, max_len=500):
        """length filter (+ PE interleave) over parse_fastx results; PE needs both parsed into ONE reads buffer, so
        p2's reads are appended behind p1's here."""
        import torch

        pe = p2 is not None
        n = p1["n"]
        dev = p1["reads"].device
        if pe:
            assert p2["n"] == n
            reads = torch.cat([p1["reads"][: p1["n_bases"]], p2["reads"][: p2["n_bases"] + 16]])
        else:
            reads = p1["reads"]
        tot = 2 * n if pe else n
        d_offs = torch.zeros(max(tot, 1), dtype=torch.int64, device=dev)
        d_lens = torch.zeros(max(tot, 1), dtype=torch.int32, device=dev)
        under, over, ml = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._ck(lib().k4_prepare_reads_dev(self.h, 1 if pe else 0, n, min_len, max_len, p1["offs"].data_ptr(),
                                            p1["lens"].data_ptr(), p2["offs"].data_ptr() if pe else None,
                                            p2["lens"].data_ptr() if pe else None, p1["n_bases"] if pe else 0,
                                            d_offs.data_ptr(), d_lens.data_ptr(), C.byref(under), C.byref(over), C.byref(ml),
                                            torch.cuda.current_stream().cuda_stream))
        return {"reads": reads, "offs": d_offs[:tot], "lens": d_lens[:tot], "n_under": under.value, "n_over": over.value,
                "max_len": ml.value, "n_units": n, "pe": pe}

    def format_sam(self, prep, p1, p2=None, rr=None, hits=None, max_ml=1, pe_recs=None, seg2=None, bam=False, sq_all=True, all_reads=False):
        """SAM body (bytes), stats dict and per-chromosome hit flags for device-resident results.  bam=True: the same
        alignments as uncompressed BAM records (k4_format_bam_dev), refIDs for a header of all (sq_all) / the hit sequences;
        all_reads=True: kalign -M1, the reads that were not accepted follow as unaligned records (k4_format_sam_all_dev)."""
        import torch

        names = SamNames()
        for w, p in enumerate([p1, p2]):
            if p is not None:
                names.d_text[w] = p["text"].data_ptr()
                names.d_name_off[w] = p["name_off"].data_ptr()
                names.d_name_len[w] = p["name_len"].data_ptr()
        d_sam, nbytes, stats = C.c_void_p(), C.c_uint64(), SamStats()
        ne = self.info()["n_entries"]
        chrom_hit = np.zeros(ne + 1, dtype=np.uint8)
        head = (self.h, 1 if prep["pe"] else 0, prep["n_units"], rr.data_ptr() if rr is not None else None,
                hits.data_ptr() if hits is not None else None, max_ml, pe_recs.data_ptr() if pe_recs is not None else None,
                seg2.data_ptr() if seg2 is not None else None, prep["reads"].data_ptr(), prep["offs"].data_ptr(),
                prep["lens"].data_ptr(), C.byref(names))
        tail = (C.byref(d_sam), C.byref(nbytes), C.byref(stats), chrom_hit.ctypes.data, torch.cuda.current_stream().cuda_stream)
        if bam:
            self._ck((lib().k4_format_bam_all_dev if all_reads else lib().k4_format_bam_dev)(*head, 1 if sq_all else 0, *tail))
        elif all_reads:
            self._ck(lib().k4_format_sam_all_dev(*head, *tail))
        else:
            self._ck(lib().k4_format_sam_ext_dev(*head, *tail))
        body = b""
        if nbytes.value:
            buf = np.empty(nbytes.value, dtype=np.uint8)
            self._ck(lib().k4_copy_to_host(self.h, buf.ctypes.data, d_sam, nbytes.value))
            body = buf.tobytes()
        lib().k4_free_device(d_sam)
        return body, {"nar": list(stats.nar), "plus": stats.plus, "minus": stats.minus, "n_lines": stats.n_lines}, chrom_hit

    def _upload(self, reads, *arrays):
        """the reads (16 zero bytes behind them), their offsets and lengths, then each of `arrays`, as device byte tensors; and the
        number of reads"""
        import torch

        dev = torch.device("cuda", self.info()["device"])
        cat, offs, lens = _flatten(reads)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        return [torch.from_numpy(np.concatenate([cat, np.zeros(16, np.uint8)])).to(dev), t(offs), t(lens)] + [t(a) for a in arrays], len(lens)

    def _records(self, reads, out, hits, pe_recs):
        """the record arguments of a report stage's entry point, `pe` to `d_lens`, over host-side results: SE (out + hits records) or
        PE (pe_recs, reads interleaved).  Returns (arguments, the tensors they point into: keep them until the call is over)."""
        if pe_recs is not None:
            keep, n = self._upload(reads, pe_recs)
            return (1, n // 2, None, None, 1, keep[3].data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()), keep
        keep, n = self._upload(reads, out, hits)
        max_ml = 1 if hits.ndim == 1 else hits.shape[1]
        return (0, n, keep[3].data_ptr(), keep[4].data_ptr(), max_ml, None, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()), keep

    def snp_csv(self, reads, out=None, hits=None, pe_recs=None, min_snp_reads=5, qvalue=0.05, snp_nonref_pcnt=25.0):
        """kalign's SNP calling (main CSV) over host-side results: SE (out + hits records) or PE (pe_recs, reads interleaved).
        Returns (CSV text, number of SNPs)."""
        rec, keep = self._records(reads, out, hits, pe_recs)
        L = lib()
        csv, nb, ns = C.c_void_p(), C.c_uint64(), C.c_uint64()
        self._ck(L.k4_snp_csv_dev(self.h, *rec, min_snp_reads, qvalue, snp_nonref_pcnt, C.byref(csv), C.byref(nb), C.byref(ns), 0))
        text = C.string_at(csv.value, nb.value).decode()
        L.k4_free_host(csv)
        return text, ns.value

    def snp_files(self, reads, out=None, hits=None, pe_recs=None, min_snp_reads=5, qvalue=0.05, snp_nonref_pcnt=25.0, vcf=False, marker_len=0,
                  marker_poly_thres=None, centroids=False):
        """every file of a kalign SNP run (k4_snp_run_dev) over host-side results, as a dict of texts: "snp" (CSV, or VCF), "wig"
        (.covsegs.wig), "disnp" (.disnp.csv), "trisnp" (.trisnp.csv), and "n_snps".  marker_len (kalign -K, 25..500; marker_poly_thres:
        --markerpolythres, default 1/3) adds "markers" (<snp file>.markers) and "n_markers"; centroids=True (kalign -7) adds
        "centroids" (k4_snp_run2_dev)."""
        rec, keep = self._records(reads, out, hits, pe_recs)
        L = lib()
        head = (self.h, 1 if vcf else 0, *rec, min_snp_reads, qvalue, snp_nonref_pcnt)
        f2 = SnpFiles2()
        f, texts = f2.files, [(f2.files, k) for k in ("snp", "wig", "disnp", "trisnp")]
        if marker_len or centroids:
            o = SnpOpts(int(marker_len), 1 if centroids else 0, DFLT_MARKER_POLY_THRES if marker_poly_thres is None else float(marker_poly_thres))
            self._ck(L.k4_snp_run2_dev(*head, C.byref(o), C.byref(f2), 0))
            texts += [(f2, k) for k, on in (("markers", marker_len), ("centroids", centroids)) if on]
        else:
            self._ck(L.k4_snp_run_dev(*head, C.byref(f), 0))
        res = {"n_snps": f.n_snps}
        if marker_len:
            res["n_markers"] = f2.n_markers
        for st, k in texts:
            res[k] = C.string_at(getattr(st, k), getattr(st, k + "_bytes")).decode()
            L.k4_free_host(getattr(st, k))
        return res

    def pba(self, reads, out=None, hits=None, pe_recs=None, experiment_id="Unspecified", readset_id="Unspecified"):
        """`ngskit4b genpba` over host-side results (k4_pba_run_dev): SE (out + hits records) or PE (pe_recs, reads interleaved).
        Returns {"pba": the .pba file's bytes, "wig": the .covsegs.wig text, "n_chroms": the number of sequence records}."""
        rec, keep = self._records(reads, out, hits, pe_recs)
        L = lib()
        f = PbaFiles()
        self._ck(L.k4_pba_run_dev(self.h, *rec, os.fsencode(experiment_id), os.fsencode(readset_id), C.byref(f), 0))
        res = {"pba": C.string_at(f.pba, f.pba_bytes), "wig": C.string_at(f.wig, f.wig_bytes).decode(), "n_chroms": f.n_chroms}
        L.k4_free_host(f.pba)
        L.k4_free_host(f.wig)
        return res

    def post_stages(self, reads, out, hits, seg2, min_flank_exacts=0, orphan_splice=False, orphan_indel=False):
        """AutoTrimFlanks / RemoveOrphanSpliceJuncts / RemoveOrphanMicroInDels (KAligner.cpp:653-686) over host arrays of SE
        results, in the reference's order; returns (out, hits, counts)."""
        n, max_ml = hits.shape
        (d_reads, d_offs, d_lens, d_rr, d_hits, d_seg2), _ = self._upload(reads, out, hits, seg2)
        cnt = {}
        c = C.c_int64(0)
        if min_flank_exacts > 0:
            self._ck(lib().k4_auto_trim_flanks_dev(self.h, min_flank_exacts, 0, n, max_ml, d_rr.data_ptr(), d_hits.data_ptr(),
                                                   d_reads.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), C.byref(c), 0))
            cnt["trim"] = c.value
        for on, which, key in ((orphan_splice, EXT_SPLICE, "splice"), (orphan_indel, EXT_INDEL, "indel")):
            if on:
                self._ck(lib().k4_remove_orphan_juncts_dev(self.h, which, n, max_ml, d_rr.data_ptr(), d_hits.data_ptr(),
                                                           d_seg2.data_ptr(), C.byref(c), 0))
                cnt[key] = c.value
        return (d_rr.cpu().numpy().view(RESULT_DTYPE), d_hits.cpu().numpy().view(HIT_DTYPE).reshape(n, max_ml), cnt)

    def reduce_pcr_dups(self, win_len, n, max_ml, d_rr, d_hits, stream=0):
        """ReducePCRduplicates (`kalign -k`, KAligner.cpp:2303-2400) in place over device arrays of SE results: d_rr (n k4_read_result
        records) and d_hits (n * max_ml k4_hit slots), torch tensors or device addresses; returns the number of reads marked NAR_PCRDUP."""
        c = C.c_int64(0)
        ptr = lambda a: a if isinstance(a, int) else a.data_ptr()  # noqa: E731
        self._ck(lib().k4_reduce_pcr_dups_dev(self.h, int(win_len), int(n), int(max_ml), ptr(d_rr), ptr(d_hits), C.byref(c), stream))
        return c.value

    def pcr5_primer_correct(self, max_subs, n, max_ml, d_reads, d_offs, d_lens, d_rr=None, d_hits=None, d_pe=None, klen=12, stream=0):
        """PCR5PrimerCorrect (`kalign -6`, KAligner.cpp:2115-2226) in place over device arrays (torch tensors or addresses): accepted
        one-segment full-length reads over (max_subs * len + 50) / 100 mismatches get the mismatching bases among their first klen
        rewritten in d_reads to the target's until they are within it, or become NAR_NOHIT.  SE d_rr + d_hits (n * max_ml slots), or PE
        d_pe (n = both ends).  Returns (reads corrected, bases corrected, reads rejected)."""
        c = (C.c_int64 * 3)()
        ptr = lambda a: None if a is None else a if isinstance(a, int) else a.data_ptr()  # noqa: E731
        pe = d_pe is not None
        self._ck(lib().k4_pcr5_primer_correct_dev(self.h, int(max_subs), int(klen), 1 if pe else 0, int(n), int(max_ml), ptr(d_pe if pe else d_rr),
                                                  ptr(d_hits), ptr(d_reads), ptr(d_offs), ptr(d_lens), c, stream))
        return tuple(int(x) for x in c)

    def load_loci_constraints(self, path):
        """LoadLociConstraints (`kalign -5 <file>`, KAligner.cpp:1363-1545): the CSV `sequence,start,end,bases` as a LOCI_CONSTRAINT_DTYPE
        array sorted by (sequence, start, end); a line the reference turns down raises K4Error (-47) with the reference's message."""
        tbl, n = C.POINTER(LociConstraint)(), C.c_int32(0)
        self._ck(lib().k4_load_loci_constraints(self.h, os.fsencode(path), C.byref(tbl), C.byref(n), None))
        try:
            if n.value == 0:
                return np.zeros(0, LOCI_CONSTRAINT_DTYPE)
            return np.frombuffer(C.string_at(tbl, n.value * C.sizeof(LociConstraint)), LOCI_CONSTRAINT_DTYPE).copy()
        finally:
            lib().k4_free_host(C.cast(tbl, C.c_void_p))

    def load_contaminants(self, path):
        """LoadContaminantsFile (`kalign -H <file>`): see the module's load_contaminants; a refusal is also left in this index's last error."""
        return load_contaminants(path, _ix=self)

    def contaminant_trims(self, contaminants, reads, reads2=None, trim5=0, trim3=0, sample_nth=1, first_unit=0):
        """k4_contam_trims_dev over host reads (PE: reads2 holds the mates): (contam5, contam3, totals) -- per read (PE: interleaved,
        2i = PE1 and 2i + 1 = PE2 of pair i) the bases a contaminant of its class overlaps the 5' / 3' end by beyond trim5 / trim3, and
        the reads with such a trim at the 5' / 3' end among PE1, then among PE2 (before any length test)."""
        import torch

        pe = reads2 is not None
        tbl = np.ascontiguousarray(contaminants, dtype=CONTAMINANT_DTYPE)
        c1, o1, l1 = _flatten(reads)
        n = len(l1)
        if pe:
            c2, o2, l2 = _flatten(reads2)
            assert len(l2) == n
        else:
            c2, o2, l2 = np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        dev = torch.device("cuda", self.info()["device"])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        d_reads = t(np.concatenate([c1, c2, np.zeros(16, np.uint8)]))
        d_o1, d_l1, d_o2, d_l2 = t(o1), t(l1), t(o2), t(l2)
        nr = 2 * n if pe else n
        d_c5 = torch.full((nr + 1,), 255, dtype=torch.uint8, device=dev)
        d_c3 = torch.full((nr + 1,), 255, dtype=torch.uint8, device=dev)
        tot = (C.c_uint64 * 4)()
        self._ck(lib().k4_contam_trims_dev(self.h, tbl.ctypes.data, len(tbl), 1 if pe else 0, n, int(trim5), int(trim3), int(sample_nth), int(first_unit),
                                           d_reads.data_ptr(), d_o1.data_ptr(), d_l1.data_ptr(), d_o2.data_ptr() if pe else None,
                                           d_l2.data_ptr() if pe else None, len(c1), d_c5.data_ptr(), d_c3.data_ptr(), tot,
                                           torch.cuda.current_stream().cuda_stream))
        assert int(d_c5[nr]) == 255 and int(d_c3[nr]) == 255  # nothing behind the last read was written
        return d_c5[:nr].cpu().numpy(), d_c3[:nr].cpu().numpy(), tuple(int(x) for x in tot)

    def chrom_accept_mask(self, include=(), exclude=()):
        """Which sequences `kalign -z <include regex> -Z <exclude regex>` keeps (CUtility::MatchExcludeRegExpr / MatchIncludeRegExpr):
        uint8[n_entries + 1] indexed by entry id, 1 = keep; an expression that does not compile raises K4Error (-100)."""
        mask = np.zeros(self.info()["n_entries"] + 1, np.uint8)
        arr = lambda xs: (C.c_char_p * max(len(xs), 1))(*[x.encode() if isinstance(x, str) else x for x in xs])  # noqa: E731
        inc, exc = list(include), list(exclude)
        self._ck(lib().k4_chrom_accept_mask(self.h, len(inc), arr(inc), len(exc), arr(exc), mask.ctypes.data))
        return mask

    def filter_chroms(self, d_accept, n, max_ml, d_rr=None, d_hits=None, d_pe=None, stream=0):
        """FiltByChroms (KAligner.cpp:4025-4091) in place over device arrays: accepted reads on a sequence whose byte in d_accept
        (uint8[n_entries + 1] on the device, see chrom_accept_mask) is 0 become NAR_CHROMFILT; SE d_rr + d_hits or PE d_pe (n records).
        Returns the number of reads marked."""
        c = C.c_int64(0)
        ptr = lambda a: None if a is None else a if isinstance(a, int) else a.data_ptr()  # noqa: E731
        pe = d_pe is not None
        self._ck(lib().k4_filter_chroms_dev(self.h, ptr(d_accept), 1 if pe else 0, int(n), int(max_ml), ptr(d_pe if pe else d_rr), ptr(d_hits),
                                            C.byref(c), stream))
        return c.value

    def filter_loci_constraints(self, constraints, n_units, max_ml, d_reads, d_offs, d_lens, d_rr=None, d_hits=None, d_seg2=None, d_pe=None,
                                stream=0):
        """IdentifyConstraintViolations (`kalign -5`, KAligner.cpp:2716-2765) in place over device arrays: constraints is a host
        LOCI_CONSTRAINT_DTYPE array (load_loci_constraints); SE n_units reads in d_rr + d_hits (+ d_seg2), PE n_units pairs in d_pe.
        Reads that violate a constraint (PE: and their mates) become NAR_LOCICONSTRAINED; returns how many."""
        c = C.c_int64(0)
        ptr = lambda a: None if a is None else a if isinstance(a, int) else a.data_ptr()  # noqa: E731
        t = np.ascontiguousarray(constraints, LOCI_CONSTRAINT_DTYPE)
        self._ck(lib().k4_filter_loci_constraints_dev(self.h, C.cast(t.ctypes.data, C.POINTER(LociConstraint)), len(t), 1 if d_pe is not None else 0,
                                                      int(n_units), int(max_ml), ptr(d_rr), ptr(d_hits), ptr(d_seg2), ptr(d_pe), ptr(d_reads),
                                                      ptr(d_offs), ptr(d_lens), C.byref(c), stream))
        return c.value

    def set_priority_regions(self, entry_ids=(), starts=(), ends=()):
        """`kalign -B`: the features as (1-based entry id, start, end), 0-based inclusive loci; none clears the table.  While a table is
        set, kalign_batch / kalign_pe_batch and the *_dev calls run ProcCoredApprox's priority pass (KAligner.cpp:9682-9770) first."""
        c = np.ascontiguousarray(entry_ids, np.uint32)
        s = np.ascontiguousarray(starts, np.uint32)
        e = np.ascontiguousarray(ends, np.uint32)
        assert len(c) == len(s) == len(e)
        self._ck(lib().k4_set_priority_regions(self.h, len(c), c.ctypes.data, s.ctypes.data, e.ctypes.data))

    def filter_priority_regions(self, n, max_ml, d_rr=None, d_hits=None, d_seg2=None, d_pe=None, stream=0):
        """FiltByPriorityRegions (KAligner.cpp:4093-4155) in place over device arrays: accepted reads whose Seg[0] span is in no feature
        of the table become NAR 12 (PR) with num_hits 0 and chrom_id 0; SE d_rr + d_hits (+ d_seg2) or PE d_pe (n records).  Returns
        the number of reads marked."""
        c = C.c_int64(0)
        ptr = lambda a: None if a is None else a if isinstance(a, int) else a.data_ptr()  # noqa: E731
        pe = d_pe is not None
        self._ck(lib().k4_filter_priority_regions_dev(self.h, 1 if pe else 0, int(n), int(max_ml), ptr(d_pe if pe else d_rr), ptr(d_hits),
                                                      ptr(d_seg2), C.byref(c), stream))
        return c.value

    def priority_select(self, n, max_ml, d_wide_rr, d_wide_hits, d_out_rr, d_out_hits, d_need, pe_mode=0, sparse_hits=False, stream=0):
        """Step (b) of the priority pass alone (KAligner.cpp:9724-9763) over device tensors: the results of a call with max_ml + 10 hit
        slots in, the settled reads' records and hits and the uint8 marks of the reads that need the normal call out.  Enqueues only."""
        self._ck(lib().k4_priority_select_dev(self.h, int(n), int(max_ml), int(pe_mode), 1 if sparse_hits else 0, d_wide_rr.data_ptr(),
                                              d_wide_hits.data_ptr(), d_out_rr.data_ptr(), d_out_hits.data_ptr(), d_need.data_ptr(), stream))

    def priority_times(self):
        """(ms of the wide pass, the select step, the normal pass; reads through the wide pass, reads that needed the normal pass)
        since the last call, while kernel timing is on"""
        ms = (C.c_double * 3)()
        rd = (C.c_uint64 * 2)()
        self._ck(lib().k4_priority_times(self.h, ms, rd))
        return tuple(ms[:]), tuple(int(x) for x in rd[:])

    def filter_marked_prior(self):
        """uint64[20]: the reads filter_chroms / filter_loci_constraints marked on this index so far, by the NAR they carried before"""
        out = (C.c_uint64 * 20)()
        self._ck(lib().k4_filter_marked_prior(self.h, out))
        return np.array(out[:], np.uint64)

    def align_stats_collect(self, on=True):
        """Start (zero) or drop the run tallies of `kalign -O` that the align calls add to: the multihit distribution and the PE insert lengths."""
        self._ck(lib().k4_align_stats_collect(self.h, 1 if on else 0))

    def align_stats(self, n, max_ml, max_read_len, d_reads, d_offs, d_lens, d_rr=None, d_hits=None, d_pe=None, stream=0, write=None):
        """The counts behind `kalign -O` (WriteSubDist, ReportTargHitCnts; KAligner.cpp:6469-6525, 5458-5712) over n reads in device arrays
        (torch tensors or addresses): SE d_rr + d_hits (n * max_ml slots), or PE d_pe (n = both ends).  Returns numpy arrays: q_insts /
        q_subs [4, max_read_len], m_sub [max_read_len + 1], multi_hit [500], pe_len_dist [100001], ent_hits / ent_uniq_loci /
        ent_indeterminate [n_entries], ent_trimer [n_entries, 64], and max_align_len, n_accepted.  write = (path, n_loaded, ml_mode,
        max_multi): also print the files."""
        ptr = lambda a: None if a is None else a if isinstance(a, int) else a.data_ptr()  # noqa: E731
        st = AlignStats()
        pe = d_pe is not None
        self._ck(lib().k4_align_stats_dev(self.h, 1 if pe else 0, int(n), int(max_ml), int(max_read_len), ptr(d_rr), ptr(d_hits), ptr(d_pe),
                                          ptr(d_reads), ptr(d_offs), ptr(d_lens), C.byref(st), stream))
        try:
            if write is not None:
                path, n_loaded, ml_mode, max_multi = write
                self._ck(lib().k4_write_align_stats(self.h, C.byref(st), int(n_loaded), int(ml_mode), int(max_multi), 1 if pe else 0,
                                                    os.fsencode(path)))
            L, ne = st.len_stride, st.n_entries
            arr = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(k,)).astype(dt).copy() if k else np.zeros(0, dt)  # noqa: E731
            return {"max_align_len": int(st.max_align_len), "n_accepted": int(st.n_accepted),
                    "q_insts": arr(st.q_insts, 4 * L, np.uint64).reshape(4, L), "q_subs": arr(st.q_subs, 4 * L, np.uint64).reshape(4, L),
                    "m_sub": arr(st.m_sub, L + 1, np.uint64), "multi_hit": arr(st.multi_hit, STATS_MULTI, np.uint64),
                    "pe_len_dist": arr(st.pe_len_dist, STATS_PE_LEN + 1, np.uint64), "ent_hits": arr(st.ent_hits, ne, np.uint32),
                    "ent_uniq_loci": arr(st.ent_uniq_loci, ne, np.uint32), "ent_indeterminate": arr(st.ent_indeterminate, ne, np.uint32),
                    "ent_trimer": arr(st.ent_trimer, ne * 64, np.uint32).reshape(ne, 64)}
        finally:
            lib().k4_free_align_stats(C.byref(st))

    def site_prefs(self, n, max_ml, ofs=-4, d_rr=None, d_hits=None, d_pe=None, stream=0, write=None):
        """The counts behind `kalign -8 <file> -9 <ofs>` (ProcessSiteProbabilites, KAligner.cpp:8708-8876) over n reads in device arrays
        (torch tensors or addresses): SE d_rr + d_hits (n * max_ml slots), or PE d_pe (n = both ends).  Returns num_occs / num_sites as
        uint32 [2, 65536] (strand, octamer) and n_accepted, n_counted.  write = path: also print the file."""
        ptr = lambda a: None if a is None else a if isinstance(a, int) else a.data_ptr()  # noqa: E731
        sp = SitePrefs()
        pe = d_pe is not None
        self._ck(lib().k4_site_prefs_dev(self.h, 1 if pe else 0, int(n), int(max_ml), int(ofs), ptr(d_rr), ptr(d_hits), ptr(d_pe), C.byref(sp),
                                         stream))
        try:
            if write is not None and lib().k4_write_site_prefs(C.byref(sp), os.fsencode(write)) != 0:
                raise K4Error(-89, lib().k4_global_error().decode())
            arr = lambda ps: np.stack([np.ctypeslib.as_array(p, shape=(65536,)).copy() for p in ps])  # noqa: E731
            return {"num_occs": arr(sp.num_occs), "num_sites": arr(sp.num_sites), "n_accepted": int(sp.n_accepted),
                    "n_counted": int(sp.n_counted)}
        finally:
            lib().k4_free_site_prefs(C.byref(sp))

    def pe_insert_dist(self, n_pairs, d_pe, stream=0, write=None):
        """The table behind `kalign -3` (ReportPEInsertLenDist, KAligner.cpp:5321-5454) over n_pairs pairs of k4_pe_read records in a
        device array (torch tensor or address; mates at 2q and 2q + 1).  Returns numpy arrays with one element per target that received
        a pair, ascending entry id: entry_id, tot_pes, median (uint32), sum (uint64), dist [n_rows, 52].  write = (path, n_accepted):
        also print the file (left empty when n_accepted is 0)."""
        pd = PeInsertDist()
        self._ck(lib().k4_pe_insert_dist_dev(self.h, int(n_pairs), d_pe if isinstance(d_pe, int) or d_pe is None else d_pe.data_ptr(),
                                             C.byref(pd), stream))
        try:
            if write is not None:
                path, n_accepted = write
                self._ck(lib().k4_write_pe_insert_dist(self.h, C.byref(pd), int(n_accepted), os.fsencode(path)))
            k = int(pd.n_rows)
            arr = lambda p, n, dt: np.ctypeslib.as_array(p, shape=(n,)).astype(dt).copy() if n else np.zeros(0, dt)  # noqa: E731
            return {"entry_id": arr(pd.entry_id, k, np.uint32), "tot_pes": arr(pd.tot_pes, k, np.uint32), "median": arr(pd.median, k, np.uint32),
                    "sum": arr(pd.sum, k, np.uint64), "dist": arr(pd.dist, k * PE_INSERT_BINS, np.uint32).reshape(k, PE_INSERT_BINS)}
        finally:
            lib().k4_free_pe_insert_dist(C.byref(pd))

    def pipeline_sam(self, texts, kp, pe=None, min_len=50, max_len=500, chunk_bytes=0, ring=False, out=None, min_batch_units=0, all_reads=False, expect=True):
        """host text (bytes-like / pinned tensors: one for SE, two for PE) -> SAM body through the overlapped pipeline.
        ring=True feeds through acquire / submit (what k4align's reader threads do), else submit_host.  Returns (body or
        number of bytes written into `out`, stats dict, view)."""
        L = lib()
        prm = PipelineParams()
        prm.paired = 1 if len(texts) == 2 else 0
        prm.kp = kp
        if pe is not None:
            prm.pe = pe
        prm.min_len, prm.max_len, prm.chunk_bytes = min_len, max_len, chunk_bytes
        prm.min_batch_units = min_batch_units  # 0: the default (4 M); small values make several alignment batches of a small input
        bufs = []
        for e, t in enumerate(texts):
            if hasattr(t, "data_ptr"):
                bufs.append((t.data_ptr(), t.numel(), t))
            else:
                a = np.frombuffer(bytes(t), dtype=np.uint8)
                bufs.append((a.ctypes.data, len(a), a))
            prm.expect_text_bytes[e] = bufs[-1][1] if expect else 0  # (unknown sizes: the arrays grow by doubling)
        pl = C.c_void_p()
        self._ck(L.k4_pipeline_open(self.h, C.byref(prm), C.byref(pl)))
        try:
            if ring:
                pos = [0] * len(bufs)
                done = [False] * len(bufs)
                while not all(done):
                    for e, (ptr, n, _) in enumerate(bufs):
                        if done[e]:
                            continue
                        b, cap = C.c_void_p(), C.c_uint64()
                        self._ck(L.k4_pipeline_acquire(pl, e, C.byref(b), C.byref(cap)))
                        ln = min(cap.value, n - pos[e])
                        C.memmove(b.value, ptr + pos[e], ln)
                        pos[e] += ln
                        done[e] = pos[e] == n
                        self._ck(L.k4_pipeline_submit(pl, e, ln, 1 if done[e] else 0))
            else:
                for e, (ptr, n, _) in enumerate(bufs):
                    self._ck(L.k4_pipeline_submit_host(pl, e, ptr, n, 1))
            view = PipelineView()
            self._ck(L.k4_pipeline_wait_aligned(pl, C.byref(view)))
            stats, nbytes = SamStats(), C.c_uint64()
            self._ck((L.k4_pipeline_format_all if all_reads else L.k4_pipeline_format)(pl, C.byref(stats), None, C.byref(nbytes)))
            st = {"nar": list(stats.nar), "plus": stats.plus, "minus": stats.minus, "n_lines": stats.n_lines,
                  "n_units": view.n_units, "n_under": view.n_under, "n_over": view.n_over, "sam_bytes": nbytes.value}
            if out is not None:
                got = C.c_uint64()
                self._ck(L.k4_pipeline_read_sam(pl, out.data_ptr(), out.numel(), C.byref(got)))
                return got.value, st, None
            parts = []
            while True:
                p, n = C.c_void_p(), C.c_uint64()
                self._ck(L.k4_pipeline_next_sam(pl, C.byref(p), C.byref(n)))
                if n.value == 0:
                    break
                parts.append(C.string_at(p.value, n.value))
            return b"".join(parts), st, None
        finally:
            L.k4_pipeline_close(pl)

    # -- the hot path (device buffers; pointers are ints, e.g. torch.Tensor.data_ptr()) -------------------------
    def kalign_pe_batch_dev(self, params, pe_params, n_pairs, max_read_len, d_reads, d_offs, d_lens, d_out, stream=0):
        self._ck(lib().k4_kalign_pe_batch_dev(self.h, C.byref(params), C.byref(pe_params), n_pairs, max_read_len,
                                              d_reads, d_offs, d_lens, d_out, stream))

    def select_hits_dev(self, n, max_ml, d_rr, d_hits, d_choice, stream=0):
        """MLMode eMLrand (`-r2`, KAligner.cpp:9945-9962): keep hits[choice % NumHits] of every accepted read."""
        self._ck(lib().k4_select_hits_dev(self.h, n, max_ml, d_rr, d_hits, d_choice, stream))

    def assign_multi(self, out, hits, ml_mode, max_reads_len):
        """CKAligner::AssignMultiMatches (`-r3` / `-r4`, KAligner.cpp:5092) over kalign_batch(pe_mode=1) results held in
        host arrays; returns (out, hits, reads assigned)."""
        import torch

        dev = torch.device("cuda", self.info()["device"])
        n, max_ml = hits.shape
        d_rr = torch.from_numpy(out.view(np.uint8).copy()).to(dev)
        d_hits = torch.from_numpy(hits.reshape(-1).view(np.uint8).copy()).to(dev)
        na = C.c_int64(0)
        self._ck(lib().k4_assign_multi_dev(self.h, ml_mode, max_reads_len, n, max_ml, d_rr.data_ptr(), d_hits.data_ptr(),
                                           C.byref(na), 0))
        return (d_rr.cpu().numpy().view(RESULT_DTYPE), d_hits.cpu().numpy().view(HIT_DTYPE).reshape(n, max_ml), na.value)

    def select_hits(self, out, hits, choice):
        """select_hits_dev over host arrays (kalign_batch's out / hits, uint32 draws); returns the new (out, hits)."""
        import torch

        dev = torch.device("cuda", self.info()["device"])
        n, max_ml = hits.shape
        d_rr = torch.from_numpy(out.view(np.uint8).copy()).to(dev)
        d_hits = torch.from_numpy(hits.reshape(-1).view(np.uint8).copy()).to(dev)
        d_ch = torch.from_numpy(np.ascontiguousarray(choice, dtype=np.uint32).view(np.int32)).to(dev)
        self.select_hits_dev(n, max_ml, d_rr.data_ptr(), d_hits.data_ptr(), d_ch.data_ptr())
        torch.cuda.synchronize()
        return (d_rr.cpu().numpy().view(RESULT_DTYPE), d_hits.cpu().numpy().view(HIT_DTYPE).reshape(n, max_ml))

    def kalign_batch_dev(self, params, n, max_read_len, d_reads, d_offs, d_lens, d_out, d_hits, stream=0):
        self._ck(lib().k4_kalign_batch_dev(self.h, C.byref(params), n, max_read_len, d_reads, d_offs, d_lens, d_out,
                                           d_hits, stream))

    def kalign_ext_batch_dev(self, params, n, max_read_len, d_reads, d_offs, d_lens, d_out, d_hits, d_seg2, stream=0):
        self._ck(lib().k4_kalign_ext_batch_dev(self.h, C.byref(params), n, max_read_len, d_reads, d_offs, d_lens, d_out, d_hits,
                                               d_seg2, stream))

    def align_reads_batch_dev(self, params, n, max_read_len, d_reads, d_offs, d_lens, d_rslt, d_inst, d_low, d_nxt,
                              d_hits, stream=0):
        self._ck(lib().k4_align_reads_batch_dev(self.h, C.byref(params), n, max_read_len, d_reads, d_offs, d_lens,
                                                d_rslt, d_inst, d_low, d_nxt, d_hits, stream))


def pe_insert_bin_host(tlen):
    """The column (0..51) of `kalign -3`'s table an insert length is counted in (k4_pe_insert_bin_host; needs the library, no GPU)."""
    return int(lib().k4_pe_insert_bin_host(int(tlen)))


def load_contaminants(path, _ix=None):
    """LoadContaminantsFile (`kalign -H <file>`, libkit4b/Contaminants.cpp:211-443): the flank contaminants of a multi-FASTA (plain or
    gzip) as a CONTAMINANT_DTYPE array, one element per (record, class), by class and falling length.  A file the reference turns down
    raises K4Error with its sentence; a `&` (vector) record raises K4Error (-3).  Needs the library, no GPU and no index."""
    tbl, n = C.POINTER(Contaminant)(), C.c_int32(0)
    err = C.create_string_buffer(256)
    rc = lib().k4_load_contaminants(_ix.h if _ix is not None else None, os.fsencode(path), C.byref(tbl), C.byref(n), err)
    if rc != 0:
        raise K4Error(rc, err.value.decode("latin-1"))
    try:
        return np.frombuffer(C.string_at(tbl, n.value * C.sizeof(Contaminant)), CONTAMINANT_DTYPE).copy()
    finally:
        lib().k4_free_host(C.cast(tbl, C.c_void_p))


def contam_match_host(contaminants, cls, min_overlap, read_bases):
    """MatchContaminants as the plain rule (k4_contam_match_host): the largest overlap >= max(min_overlap, 1) of a contaminant of class
    cls (0..3) onto the read's 5' (classes 0, 1) or 3' end, 0 for none.  read_bases: etSeqBase bytes.  Needs the library, no GPU."""
    tbl = np.ascontiguousarray(contaminants, dtype=CONTAMINANT_DTYPE)
    rd = np.ascontiguousarray(read_bases, dtype=np.uint8)
    rc = int(lib().k4_contam_match_host(tbl.ctypes.data if len(tbl) else None, len(tbl), int(cls), int(min_overlap), rd.ctypes.data if len(rd) else None, len(rd)))
    if rc < 0:
        raise K4Error(rc, "k4_contam_match_host")
    return rc


def pe_insert_median_host(values):
    """CKAligner::MedianInsertLen (KAligner.cpp:5256-5319) of a target's insert lengths in walk order, by the function the kernel runs
    (k4_pe_insert_median_host; needs the library, no GPU).  values: uint32, none of them 0."""
    values = np.ascontiguousarray(values, np.uint32)
    med = C.c_uint32(0)
    rc = lib().k4_pe_insert_median_host(values.ctypes.data, len(values), C.byref(med))
    if rc != 0:
        raise K4Error(rc, "k4_pe_insert_median_host")
    return int(med.value)


def pba_classify_host(cnt7, ref_bases):
    """genpba's per-locus rule on the host (k4_pba_classify_host; needs the library, no GPU).  cnt7: uint32 array [7, n_loci] -- the
    reference count, the non-reference count and the non-reference counts of A, C, G, T, N; ref_bases: the target's symbol per locus.
    Returns (PBA bytes, coverage) as uint8 / uint32 arrays."""
    cnt7 = np.ascontiguousarray(cnt7, dtype=np.uint32)
    ref_bases = np.ascontiguousarray(ref_bases, dtype=np.uint8)
    if cnt7.ndim != 2 or cnt7.shape[0] != 7 or ref_bases.shape != (cnt7.shape[1],):
        raise ValueError("cnt7 is [7, n_loci], ref_bases [n_loci]")
    n = cnt7.shape[1]
    pba, cov = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    rc = lib().k4_pba_classify_host(cnt7.ctypes.data, n, n, ref_bases.ctypes.data, pba.ctypes.data, cov.ctypes.data)
    if rc != 0:
        raise K4Error(rc, "k4_pba_classify_host")
    return pba, cov


def marker_classify_host(cnt7, ref_bases, min_snp_reads, poly_thres=DFLT_MARKER_POLY_THRES):
    """the per-locus rule of kalign's marker sequences on the host (k4_marker_classify_host; needs the library, no GPU).  cnt7 and
    ref_bases as for pba_classify_host.  Returns (base, polymorphic) as uint8 arrays: base 0..4 = A, C, G, T, N, 0xff = fewer than
    min_snp_reads bases there, 0xfe = no allele reaches 1 - poly_thres (both reject the marker)."""
    cnt7 = np.ascontiguousarray(cnt7, dtype=np.uint32)
    ref_bases = np.ascontiguousarray(ref_bases, dtype=np.uint8)
    if cnt7.ndim != 2 or cnt7.shape[0] != 7 or ref_bases.shape != (cnt7.shape[1],):
        raise ValueError("cnt7 is [7, n_loci], ref_bases [n_loci]")
    n = cnt7.shape[1]
    base, poly = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    rc = lib().k4_marker_classify_host(cnt7.ctypes.data, n, n, ref_bases.ctypes.data, int(min_snp_reads), float(poly_thres), base.ctypes.data,
                                       poly.ctypes.data)
    if rc != 0:
        raise K4Error(rc, "k4_marker_classify_host")
    return base, poly


def build_sa_device(concat_len, el_size, d_seq_ptr, d_sa_ptr, device=0):
    """GPU suffix sort (CSfxArray::Finalise -> QSortSeq, SfxArray.cpp:1758,9739)."""
    rc = lib().k4_build_sa_device(concat_len, el_size, d_seq_ptr, d_sa_ptr, device)
    if rc != 0:
        raise K4Error(rc, lib().k4_global_error().decode())
