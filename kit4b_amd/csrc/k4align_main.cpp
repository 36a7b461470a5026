// kit4b_amd/csrc/k4align_main.cpp -- `k4align`: the stand-alone counterpart of `ngskit4b kalign` for the accelerated path.
//
// Host C++ over the C ABI of libk4sfx.so only (no HIP here): the files are read (and inflated) on the host, everything
// between the raw text and the SAM body runs on the device.  Mirrors, for the default SAM report mode:
//   reads loading        CKAligner::LoadRawReads    ngskit4b/KAligner.cpp:11648-12421 (FASTA/FASTQ, .gz, length filter,
//                                                   descriptor = first token, bases to etSeqBase) -> k4_parse_fastx_dev,
//                                                   k4_prepare_reads_dev
//   align phase          CKAligner::ProcCoredApprox ngskit4b/KAligner.cpp:10110-10263  -> k4_kalign_batch_dev
//   PE pass              CKAligner::ProcessPairedEnds :2944-3596                      -> k4_kalign_pe_batch_dev
//   statistics           CKAligner::ReportAlignStats :3600-3830 (NAR histogram, strand counts)
//   SAM                  CKAligner::WriteBAMReadHits :5718-5914, ReportBAMread :5957-6320, SortHitMatch :10969,
//                        CSAMfile::AddAlignment libkit4b/SAMfile.cpp:2194-2377 -> k4_format_sam_dev; header :1615,1667-1669,1799
//   PCR duplicates (-k)  CKAligner::ReducePCRduplicates :2303-2400                -> k4_reduce_pcr_dups_dev
//   5' primer correction (-6) CKAligner::PCR5PrimerCorrect :2115-2226 (aligned with min(-s + n, 15), :245-248; behind -k, in front of -x)
//                                                                                  -> k4_pcr5_primer_correct_dev
//   statistics files (-O) CKAligner::WriteSubDist :6469-6525, WriteBasicCountStats :4159-4300, ReportTargHitCnts :5458-5712,
//                        the insert size file of ProcessPairedEnds :3092-3146     -> k4_pipeline_align_stats, k4_write_align_stats
//   PE insert lengths per target (-3, with -O) CKAligner::ReportPEInsertLenDist :5321-5454, MedianInsertLen :5256-5319
//                                                                                  -> k4_pipeline_pe_insert_dist, k4_write_pe_insert_dist
//   loci constraints (-5) CKAligner::LoadLociConstraints :1363-1545, IdentifyConstraintViolations :2716-2765
//                                                                                  -> k4_load_loci_constraints, k4_filter_loci_constraints_dev
//   site preferences (-8, -9) CKAligner::ProcessSiteProbabilites :8708-8876, WriteSitePrefs :8910-8945
//                                                                                  -> k4_pipeline_site_prefs, k4_write_site_prefs
//   chromosome filters   CKAligner::FiltByChroms :4025-4091 (kalign -Z / -z; here --chromexclude / --chromeinclude)
//                                                                                  -> k4_chrom_accept_mask, k4_filter_chroms_dev
// Options follow kalign's letters: -i -u -I -o -s -e -m -n -U -d -D -E -l -L -r -R -X -N -c -a -A -x -k -6 -O -3 -5 -8 -9 -g (plus -@ <gpu>, -S <i/N> read slice);
// kalign's -Z / -z go by their long names --chromexclude / --chromeinclude (the letters mean something else here).
#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include <algorithm>
#include <atomic>
#include <thread>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <map>
#include <queue>
#include <regex>
#include <memory>
#include <string>
#include <vector>
#include <sys/mman.h>
#include <sys/wait.h>
#include "../../include/k4comm.h"
#include "../../include/k4sfx.h"
#include "../../include/k4_bam.hpp"
#include "k4_merge.h"
#include "k4_priority_bed.h"

namespace {

struct Opts {
  std::vector<std::string> in1, in2;  // -i / -u may repeat: the files are read one after the other (KAlignerCL.cpp: up to cRRMaxInFiles)
  std::string sfx, out;
  int max_subs = 5, min_edit = 1, pmode = 0, max_ns = 1, pe_mode = 0, pair_min = 100, pair_max = -1 /* not given */, pair_strand = 0;
  int min_len = 50, max_len = 500;  // cDfltMinAcceptReadLen / cDfltMaxAcceptReadLen, KAligner.h:112-113
  int ml_mode = 0, max_multi = 0;   // -r / -R (etMLMode, KAligner.h:250-258)
  bool clamp = false, best = false; // -X / -N (KAlignerCL.cpp:278-280)
  int q_method = 3;  // -g (etFQMethod, KAlignerCL.cpp:241,499): 3 = the quality lines are ignored
  int min_chimeric = 0, micro_indel = 0, splice_junct = 0, min_flank_exacts = 0;  // -c / -a / -A / -x (KAlignerCL.cpp:237,245,246,267)
  int pcr_win = -1;                 // -k <0..250>: PCR artefact reduction window (KAlignerCL.cpp:222,738-743); -1 = off
  bool pcr_given = false;           // (an explicit -k-1 is turned down like any value outside 0..250)
  int primer_subs = 0;              // -6 / --pcrprimersubs <0..5>: align with -s + n, then correct 5' primer artefacts back to -s (KAlignerCL.cpp:268,803-815); 0 = off
  std::string loci_file;            // -5 / --lociconstraints <file>: loci base constraints CSV (KAlignerCL.cpp:255)
  std::vector<std::string> chrom_excl, chrom_incl;  // --chromexclude / --chromeinclude <regex>, each repeatable (kalign -Z / -z, KAlignerCL.cpp:274-275)
  std::string priority_file;        // --priorityregionfile <bed>: kalign's -B (KAlignerCL.cpp:1095-1106; -B is the chunk size here)
  bool no_filt_priority = false;    // -V / --nofiltpriority: FiltByPriorityRegions is left out; without a file it does nothing
  std::string stats_file;           // -O <file>: alignment statistics (KAlignerCL.cpp:256) and its two side files
  bool pe_insert_dist = false;      // -3 / --petranslendist: per-target PE insert length distributions into <-O file>.peinserts.csv (KAlignerCL.cpp:288)
  std::string site_file;            // -8 / --siteprefs <file>: start-site octamer preferences (KAlignerCL.cpp:252)
  int site_ofs = -4;                // -9 / --siteprefsofs <-100..100>: cDfltRelSiteStartOfs (KAlignerCL.cpp:253,1053)
  double batch_mb = 0;              // -b <MB>: stream the input, this much text per file per batch (0: the whole input at once)
  int shard = 0, n_shards = 1;      // -S i/N: this process aligns the i-th of N contiguous slices of the reads (one process per GPU)
  int gpu = 0;
  std::vector<int> gpus;            // -G g0,g1,...: one rank process per listed GPU (RCCL over xGMI, libk4comm.so)
  int rank = 0, n_ranks = 1;        // this process's place in a -G run
  bool rank_bam = false;            // ... whose output is a BAM file: the rank leaves its sorted records (all sequences numbered) + a dictionary beside them
  struct MultiShared* shared = nullptr;
  int print_slices = 0;             // -W <n>: print the byte offsets -G would cut the reads files at for n ranks, and stop (no GPU needed)
  int rpt_sq_thres = 10000;         // -4 <n>: with more reference sequences than this only those with alignments are declared in the header (KAlignerCL.cpp:289,868-870)
  std::string none_file, multi_file; // -j / -J <file>: the reads without an alignment / the multi-aligned reads as FASTA (KAlignerCL.cpp:254-255)
  int sample_nth = 1;               // -# <n>: every n-th read / pair of the input is processed (KAlignerCL.cpp:244,484-489)
  int trim5 = 0, trim3 = 0;         // -y / -Y <n>: bases taken off the 5' / 3' end of every read when loading (KAlignerCL.cpp:763-774)
  std::string contam_file;          // -H / --contaminants <file>: flank contaminants trimmed off the read ends when loading (KAlignerCL.cpp:251)
  k4_contaminant* contam_tbl = nullptr;  // ... loaded before anything touches a device (KAligner.cpp:284-301); lives as long as the process
  int32_t n_contam_tbl = 0;
  int align_strand = 0;             // -Q <0|1|2>: align to either strand, the sense or the antisense strand only (KAlignerCL.cpp:241,491)
  int fmode = 0;                    // -M <0|1|3>: 0 SAM / BAM with the accepted alignments, 1 SAM with every loaded read (KAlignerCL.cpp:217),
                                    // 3 no SAM: -o is genpba's packed base alleles file (kalignerPBA, KAlignerCL.cpp:1540-2290)
  std::string experiment_id, readset_id;  // --experimentid / --readsetid <str>: genpba's -w / -W (KAlignerCL.cpp:1617-1618), required with -M3
  std::string given;                // the option letters of the command line (genpba's argument table is narrower than kalign's)
  bool legacy = false;              // -Z: the serial whole-input path of round 1 (one batch, no overlap), kept for comparison
  int chunk_mb = 256;               // -B <MB>: size of one pinned upload buffer of the pipeline
  int io_threads = 8;               // -t <n>: concurrent pread / pwrite calls per buffer; BAM: deflate threads
  int min_snp_reads = 0;            // -p <n> (0: no SNP calling), -P <qvalue>, -1 <pct>, -S <file> (KAlignerCL.cpp:259,284-291,877-932)
  double qvalue = 0.0, snp_nonref_pcnt = 25.0;
  std::string snp_file;
  std::string cent_file;            // -7 / --snpcentroid <file>: SNP centroid distribution (KAlignerCL.cpp:260,976-983)
  int marker_len = 0;               // -K / --markerlen <25..500>: marker sequences to <snp file>.markers (KAlignerCL.cpp:261,949-960)
  bool marker_thres_given = false;
  double marker_poly_thres = 0.0;   // --markerpolythres <0.0..0.5> (kalign's -G; here -G is the GPU list): cDfltMinMarkerSNPProp when not given
  int bam_level = 6;                // -z <0..9>: BGZF deflate level of a .bam output (WriteBAMReadHits is called with 6, KAligner.cpp:759)
};

// a device block of the program's own: freed when its holder goes, whatever way the function that allocated it is left
struct DevFree { void operator()(void* p) const { k4_free_device(p); } };
typedef std::unique_ptr<void, DevFree> DevBlock;
int alloc_dev(k4_index* ix, uint64_t bytes, DevBlock& b) {
  void* p = nullptr;
  const int rc = k4_alloc_device(ix, bytes, &p);
  b.reset(p);
  return rc;
}

struct Parsed {  // one reads file after k4_parse_fastx_dev: everything lives in HBM
  DevBlock text, offs, lens, noff, nlen;
  uint64_t n = 0, bases = 0;
  uint32_t max_len = 0;
};

#define CK(call)                                                          \
  do {                                                                    \
    int _rc = (call);                                                     \
    if (_rc != K4_OK) {                                                   \
      fprintf(stderr, "k4align: %s (%d)\n", k4_last_error(ix), _rc);      \
      return _rc;                                                         \
    }                                                                     \
  } while (0)

typedef std::chrono::steady_clock::time_point TimePoint;
TimePoint now() { return std::chrono::steady_clock::now(); }
double secs(TimePoint a, TimePoint b) { return std::chrono::duration<double>(b - a).count(); }

// upload the text and parse it on the device, in pieces below the 4 GiB limit of one call; at most max_records records;
// *consumed = text bytes that belonged to them (the rest is resubmitted in front of the next batch)
int load_reads(k4_index* ix, const uint8_t* text, uint64_t T, int final_text, int64_t max_records, void* d_reads, uint64_t reads_base,
               Parsed& P, uint64_t* consumed) {
  *consumed = 0;
  if (T == 0) return K4_OK;
  const bool fastq = text[0] == '@';
  const uint64_t nl = (uint64_t)std::count(text, text + T, (uint8_t)'\n');
  const int64_t cap = std::min<int64_t>((int64_t)((nl + 1) / (fastq ? 4 : 2) + 4), max_records > 0 ? max_records : INT64_MAX);
  CK(alloc_dev(ix, T + 16, P.text));
  CK(k4_copy_to_device(ix, P.text.get(), text, T));
  CK(alloc_dev(ix, (uint64_t)cap * 8, P.offs));
  CK(alloc_dev(ix, (uint64_t)cap * 4, P.lens));
  CK(alloc_dev(ix, (uint64_t)cap * 8, P.noff));
  CK(alloc_dev(ix, (uint64_t)cap * 4, P.nlen));
  uint64_t pos = 0;
  const uint64_t piece = 3ull << 30;
  int fmt = 0;
  while (pos < T && (int64_t)P.n < cap) {
    const uint64_t len = std::min(piece, T - pos);
    const int final_chunk = final_text && pos + len == T;
    k4_parse_info info;
    CK(k4_parse_fastx_dev(ix, (const uint8_t*)P.text.get() + pos, len, pos, final_chunk, fmt, cap - (int64_t)P.n, d_reads,
                          reads_base + P.bases, (uint8_t*)P.offs.get() + 8 * P.n, (uint8_t*)P.lens.get() + 4 * P.n,
                          (uint8_t*)P.noff.get() + 8 * P.n, (uint8_t*)P.nlen.get() + 4 * P.n, &info, nullptr));
    if (info.format) fmt = (int)info.format;
    if (info.consumed == 0) break;  // nothing but an incomplete tail
    P.n += info.n_records;
    P.bases += info.n_bases;
    P.max_len = std::max(P.max_len, info.max_len);
    pos += info.consumed;
  }
  *consumed = pos;
  return K4_OK;
}

// the reads files of one end, read in portions as one text (a file that lacks its last newline gets one): buf holds the
// text not yet consumed
struct Stream {
  gzFile f = nullptr;
  std::vector<std::string> paths;
  size_t next = 0;
  std::vector<uint8_t> buf;
  bool eof = false;
  bool open_next() {
    if (f) gzclose(f);
    f = gzopen(paths[next++].c_str(), "rb");
    if (f) gzbuffer(f, 1 << 20);
    return f != nullptr;
  }
  bool open(const std::vector<std::string>& files) {
    paths = files;
    for (const std::string& q : paths) {  // all of them must be readable before anything is aligned
      FILE* t = fopen(q.c_str(), "rb");
      if (!t) { fprintf(stderr, "k4align: unable to open '%s'\n", q.c_str()); return false; }
      fclose(t);
    }
    return !paths.empty() && open_next();
  }
  bool fill(uint64_t want) {  // until buf holds `want` bytes or the file ends
    while (!eof && buf.size() < want) {
      const size_t old = buf.size();
      const size_t step = (size_t)std::min<uint64_t>(std::max<uint64_t>(want - old, 1 << 20), 256u << 20);
      buf.resize(old + step);
      const int got = gzread(f, buf.data() + old, (unsigned)step);
      if (got < 0) return false;
      buf.resize(old + (size_t)got);
      if (got == 0) {
        if (next == paths.size()) { eof = true; break; }
        if (!buf.empty() && buf.back() != '\n') buf.push_back('\n');
        if (!open_next()) return false;
      }
    }
    return true;
  }
  void drop(uint64_t n) { buf.erase(buf.begin(), buf.begin() + (ptrdiff_t)std::min<uint64_t>(n, buf.size())); }
  void close() { if (f) gzclose(f); f = nullptr; }
  ~Stream() { close(); }
};

// ---- the pipelined (default) mode: one reader thread per end fills the library's pinned ring buffers ----------------------
bool is_gzip(const std::string& path) {
  unsigned char m[2] = {0, 0};
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  const size_t got = fread(m, 1, 2, f);
  fclose(f);
  return got == 2 && m[0] == 0x1f && m[1] == 0x8b;
}
uint64_t file_size(const std::string& path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0 ? (uint64_t)st.st_size : 0;
}
// [off, off + len) of a file read into, or written from, `mem` by nt threads side by side (tmpfs / the page cache deliver and
// take more than one thread can move); less than 8 MB goes in one piece
template <bool kWrite> bool io_parallel(int fd, uint8_t* mem, uint64_t off, uint64_t len, int nt) {
  if (len < (8u << 20) || nt < 1) nt = 1;
  std::atomic<bool> ok(true);
  auto part = [&](int t) {
    const uint64_t b = len * (uint64_t)(t + 1) / nt;
    for (uint64_t done = len * (uint64_t)t / nt; done < b;) {
      const ssize_t g = kWrite ? pwrite(fd, mem + done, b - done, (off_t)(off + done)) : pread(fd, mem + done, b - done, (off_t)(off + done));
      if (g <= 0) { ok = false; return; }
      done += (uint64_t)g;
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(part, t);
  part(0);
  for (std::thread& x : th) x.join();
  return ok;
}
// One end's text on its way into the pipeline's pinned ring buffers: room for bytes (or put), the newline a file lacks, the
// final chunk.  The clock is the reading time: it stands still while the writer waits for a free buffer or hands one over.
struct ChunkWriter {
  k4_pipeline* pl;
  int end;
  void* buf = nullptr;
  uint64_t cap = 0, used = 0;
  uint8_t last = '\n';  // the last byte written
  double busy = 0;
  TimePoint t0 = now();
  ChunkWriter(k4_pipeline* p, int e) : pl(p), end(e) {}
  int room(uint8_t** p, uint64_t* n) {  // at least one free byte
    if (!buf) {
      busy += secs(t0, now());
      const int rc = k4_pipeline_acquire(pl, end, &buf, &cap);
      t0 = now();
      used = 0;
      if (rc != K4_OK) return rc;
    }
    *p = (uint8_t*)buf + used;
    *n = cap - used;
    return K4_OK;
  }
  int wrote(uint64_t n, int fin = 0) {  // n bytes of the room were filled; a full buffer (or the final one) goes to the pipeline
    used += n;
    if (n) last = ((uint8_t*)buf)[used - 1];
    if (used < cap && !fin) return K4_OK;
    busy += secs(t0, now());
    const int rc = k4_pipeline_submit(pl, end, used, fin);
    t0 = now();
    buf = nullptr;
    used = 0;
    return rc;
  }
  int put(const uint8_t* src, uint64_t n) {
    while (n) {
      uint8_t* p;
      uint64_t free_bytes;
      int rc = room(&p, &free_bytes);
      if (rc != K4_OK) return rc;
      const uint64_t take = std::min(n, free_bytes);
      memcpy(p, src, take);
      src += take; n -= take;
      if ((rc = wrote(take)) != K4_OK) return rc;
    }
    return K4_OK;
  }
  int end_file(bool more) {  // text follows a file that lacks its last newline: the next record starts on a line of its own
    const uint8_t nl = '\n';
    return more && last != '\n' ? put(&nl, 1) : K4_OK;
  }
  int finish(int rc, double* secs_read) {  // the final (possibly empty) chunk still has to be announced
    uint8_t* p;
    uint64_t n;
    if (rc == K4_OK && (rc = room(&p, &n)) == K4_OK) rc = wrote(0, 1);
    if (secs_read) *secs_read = busy + secs(t0, now());
    return rc;
  }
};

struct FileRange { std::string path; uint64_t a, b, file_len; };  // the bytes [a, b) of an uncompressed file
int feed_range(ChunkWriter& w, const FileRange& fr, int io_threads) {
  const int fd = open(fr.path.c_str(), O_RDONLY);
  if (fd < 0) return K4_ERR_OPEN_FILE;
  int rc = K4_OK;
  uint8_t* p;
  uint64_t n;
  for (uint64_t pos = fr.a; pos < fr.b && rc == K4_OK && (rc = w.room(&p, &n)) == K4_OK; pos += n) {
    n = std::min(n, fr.b - pos);
    rc = io_parallel<false>(fd, p, pos, n, io_threads) ? w.wrote(n) : K4_ERR_FILE_ACCESS;
  }
  close(fd);
  return rc;
}
int feed_gzip(ChunkWriter& w, const std::string& path) {
  gzFile g = gzopen(path.c_str(), "rb");
  if (!g) return K4_ERR_OPEN_FILE;
  gzbuffer(g, 4u << 20);
  int rc = K4_OK, got = 1;
  uint8_t* p;
  uint64_t n;
  while (rc == K4_OK && got > 0 && (rc = w.room(&p, &n)) == K4_OK) {  // (0: the end of this file)
    got = gzread(g, p, (unsigned)std::min<uint64_t>(n, 1u << 30));
    rc = got < 0 ? K4_ERR_FILE_ACCESS : w.wrote((uint64_t)got);
  }
  gzclose(g);
  return rc;
}
// every file of one end, in order, into the pipeline; a file that lacks its last newline gets one (as Stream does)
int feed_end(k4_pipeline* pl, int end, const std::vector<std::string>& files, int io_threads, double* secs_read) {
  ChunkWriter w(pl, end);
  int rc = K4_OK;
  for (size_t f = 0; f < files.size() && rc == K4_OK; f++) {
    const uint64_t len = file_size(files[f]);
    rc = is_gzip(files[f]) ? feed_gzip(w, files[f]) : feed_range(w, FileRange{files[f], 0, len, len}, io_threads);
    if (rc == K4_OK) rc = w.end_file(f + 1 < files.size());
  }
  return w.finish(rc, secs_read);
}

// ---- k4align -G: one rank process per GPU ---------------------------------------------------------------------------------------
#define K4_MAX_RANKS 64
#define K4_MAX_FILES 64  // reads files per end a -G run may name
struct MultiShared {  // an anonymous shared mapping the parent creates before it forks the ranks
  uint8_t id[K4_COMM_ID_BYTES];
  std::atomic<int> id_ready, slices_ready, failed;
  // byte offsets of the ranks' record slices in every reads file of each end: rank r reads [off[r], off[r + 1]) of file f
  uint64_t slice_off[2][K4_MAX_FILES][K4_MAX_RANKS + 1];
  uint64_t n_records;
};

// One uncompressed FASTA / FASTQ file mapped, its record starts counted per range (pass 1, parallel); byte offsets of given
// record numbers come from a second look at the one range each falls into (pass 2).
struct RecIndex {
  const uint8_t* t = nullptr;
  uint64_t len = 0, R = 0;
  bool fastq = false;
  int nt = 1;
  std::vector<uint64_t> part;  // marks in front of range k (a mark starts a record: FASTA -- '>' at a line start; FASTQ -- every line)
  ~RecIndex() { if (t && len) munmap((void*)t, len); }
  uint64_t count(uint64_t a, uint64_t b) const {  // FASTA: header lines starting in [a, b); FASTQ: newlines in [a, b)
    uint64_t c = 0;
    if (fastq) {
      const uint8_t* p = t + a;
      while (p < t + b) { const void* q = memchr(p, '\n', (size_t)(t + b - p)); if (!q) break; c++; p = (const uint8_t*)q + 1; }
    } else {
      for (uint64_t p = a; p < b;) {
        const void* q = memchr(t + p, '>', (size_t)(b - p));
        if (!q) break;
        const uint64_t at = (uint64_t)((const uint8_t*)q - t);
        if (at == 0 || t[at - 1] == '\n') c++;
        p = at + 1;
      }
    }
    return c;
  }
  bool open_file(const std::string& path, int threads) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    len = file_size(path);
    nt = std::max(threads, 1);
    part.assign((size_t)nt + 1, 0);
    if (len == 0) { close(fd); R = 0; return true; }
    t = (const uint8_t*)mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (t == MAP_FAILED) { t = nullptr; return false; }
    fastq = t[0] == '@';
    std::vector<std::thread> th;
    for (int k = 0; k < nt; k++) th.emplace_back([this, k] { part[(size_t)k + 1] = count(len * k / nt, len * (k + 1) / nt); });
    for (std::thread& x : th) x.join();
    for (int k = 0; k < nt; k++) part[(size_t)k + 1] += part[(size_t)k];
    if (fastq) { const uint64_t lines = part[(size_t)nt] + (t[len - 1] != '\n' ? 1 : 0); R = lines / 4; }
    else R = part[(size_t)nt];
    return true;
  }
  uint64_t offset_of(uint64_t rec) const {  // where record `rec` (0-based) starts; R and beyond: the end of the file
    if (rec == 0) return 0;
    if (rec >= R) return len;
    // FASTQ: the byte behind newline number 4 * rec; FASTA: the position of header number rec (0-based)
    const uint64_t target = fastq ? 4 * rec : rec + 1;  // the target-th mark (1-based) of the file
    int k = 0;
    while (k + 1 < nt && part[(size_t)k + 1] < target) k++;
    uint64_t seen = part[(size_t)k], p = len * k / nt;
    const uint64_t end = len * (k + 1) / nt;
    if (fastq) {
      while (p < end) { const void* q = memchr(t + p, '\n', (size_t)(end - p)); if (!q) break; p = (uint64_t)((const uint8_t*)q - t) + 1; if (++seen == target) return p; }
    } else {
      while (p < end) {
        const void* q = memchr(t + p, '>', (size_t)(end - p));
        if (!q) break;
        const uint64_t a2 = (uint64_t)((const uint8_t*)q - t);
        if ((a2 == 0 || t[a2 - 1] == '\n') && ++seen == target) return a2;
        p = a2 + 1;
      }
    }
    return len;
  }
};

// The records of all files of one end, taken as one sequence, cut into n_ranks contiguous slices: rank r gets the records
// [R r / N, R (r + 1) / N) (pairs stay together: both ends are cut at the same record numbers, file by file -- the two ends'
// files must hold the same numbers of records, as kalign demands of them).  offs[f][r]: where rank r starts in file f.
// counts: records per file (filled for end 0, compared for end 1).
bool slice_files(const std::vector<std::string>& files, int n_ranks, std::vector<uint64_t>& counts, bool compare_counts,
                 uint64_t (*offs)[K4_MAX_RANKS + 1], uint64_t* n_records, int nt, std::string* why) {
  std::vector<std::unique_ptr<RecIndex>> ri;
  uint64_t R = 0;
  for (size_t f = 0; f < files.size(); f++) {
    ri.emplace_back(new RecIndex);
    if (!ri.back()->open_file(files[f], nt)) { *why = "unable to read " + files[f]; return false; }
    if (compare_counts && (f >= counts.size() || counts[f] != ri.back()->R)) {
      *why = "the PE1 and PE2 files hold different numbers of reads (" + std::to_string(f < counts.size() ? counts[f] : 0) + ", " + std::to_string(ri.back()->R) + ")";
      return false;
    }
    if (!compare_counts) counts.push_back(ri.back()->R);
    R += ri.back()->R;
  }
  *n_records = R;
  uint64_t start = 0;  // records in front of file f
  for (size_t f = 0; f < files.size(); f++) {
    for (int r = 0; r <= n_ranks; r++) {
      const uint64_t g = r == n_ranks ? R : R * (uint64_t)r / (uint64_t)n_ranks;  // first record of rank r, over all files
      const uint64_t local = g <= start ? 0 : std::min<uint64_t>(g - start, ri[f]->R);
      offs[f][r] = ri[f]->offset_of(local);  // (behind the file's last record: its length, a missing final newline included)
    }
    start += ri[f]->R;
  }
  return true;
}

// the byte ranges [a, b) of uncompressed files, one after the other, into the pipeline; a range that ends a file which lacks its
// last newline gets one (the next file's first record starts on a line of its own)
int feed_ranges(k4_pipeline* pl, int end, const std::vector<FileRange>& ranges, int io_threads, double* secs_read) {
  ChunkWriter w(pl, end);
  int rc = K4_OK;
  for (size_t k = 0; k < ranges.size() && rc == K4_OK; k++) {
    const FileRange& fr = ranges[k];
    if (fr.b <= fr.a) continue;
    rc = feed_range(w, fr, io_threads);
    bool more = false;
    for (size_t q = k + 1; q < ranges.size(); q++) more |= ranges[q].b > ranges[q].a;
    if (rc == K4_OK && fr.b == fr.file_len) rc = w.end_file(more);
  }
  return w.finish(rc, secs_read);
}

// Compressed input cannot be cut by byte offsets: every rank inflates the whole stream and keeps the record blocks dealt to it --
// block number (record number / K4_DEAL_RECORDS) modulo the rank count; both ends are dealt by the same record numbers, so
// mates stay together.  (Equal sort keys then come out in block order, not in load order: the reference leaves that order open.)
#define K4_DEAL_RECORDS (1u << 18)
int feed_dealt(k4_pipeline* pl, int end, const std::vector<std::string>& files, int rank, int n_ranks, double* secs_read) {
  ChunkWriter w(pl, end);
  int rc = K4_OK;
  std::vector<uint8_t> chunk((size_t)16 << 20);
  uint64_t rec = 0;      // records begun so far, over all files
  uint32_t lines = 0;    // FASTQ: lines of the current record seen so far
  int fastq = -1;
  bool at_line_start = true;
  uint8_t last = '\n';
  auto mine_is = [&](uint64_t r) { return (r / K4_DEAL_RECORDS) % (uint64_t)n_ranks == (uint64_t)rank; };
  for (size_t f = 0; f < files.size() && rc == K4_OK; f++) {
    gzFile g = gzopen(files[f].c_str(), "rb");  // (reads plain files as they are)
    if (!g) return K4_ERR_OPEN_FILE;
    gzbuffer(g, 4u << 20);
    for (;;) {
      const int got = gzread(g, chunk.data(), (unsigned)chunk.size());
      if (got < 0) { gzclose(g); return K4_ERR_FILE_ACCESS; }
      if (got == 0) break;
      if (fastq < 0) fastq = chunk[0] == '@' ? 1 : 0;
      // runs of bytes that belong to one record block go out (or not) together
      int run_start = 0;
      bool mine = rec ? mine_is(rec - 1) : false;  // the record we are inside
      for (int q = 0; q < got && rc == K4_OK; q++) {
        const uint8_t ch = chunk[(size_t)q];
        bool starts = false;
        if (at_line_start) {
          if (fastq) { if (lines == 0) starts = true; }
          else if (ch == '>') starts = true;
        }
        if (starts) {
          const bool m2 = mine_is(rec);
          if (m2 != mine) {
            if (mine) rc = w.put(chunk.data() + run_start, (uint64_t)(q - run_start));
            run_start = q;
            mine = m2;
          }
          rec++;
        }
        at_line_start = ch == '\n';
        if (fastq && at_line_start) lines = (lines + 1) & 3u;
      }
      if (mine && rc == K4_OK) rc = w.put(chunk.data() + run_start, (uint64_t)(got - run_start));
      last = chunk[(size_t)got - 1];
      if (rc != K4_OK) break;
    }
    gzclose(g);
    if (last != '\n' && f + 1 < files.size()) {  // the next file starts on a line of its own
      const uint8_t nl = '\n';
      if (rec && mine_is(rec - 1) && rc == K4_OK) rc = w.put(&nl, 1);
      at_line_start = true;
      if (fastq == 1) lines = (lines + 1) & 3u;
      last = '\n';
    }
  }
  return w.finish(rc, secs_read);
}

const char* kNarAbbr[20] = {"NA", "AA", "EN", "NL", "MH", "ML", "ET", "OJ", "OM", "DP", "DS", "FC", "PR", "UI", "OI", "UP", "IS", "IT", "NP", "LC"};

// the front end's cleaning of an identifier (KAlignerCL.cpp:1697-1729): at most 81 characters, every quote dropped
// (CUtility::TrimQuotes), white space trimmed off both ends and every run of it inside made one space (ReduceWhitespace)
std::string clean_id(const std::string& raw) {
  std::string t;
  for (const char c : raw.substr(0, 81))
    if (c != '"' && c != '\'') t += c;
  std::string out;
  for (const char c : t) {
    if (!isspace((unsigned char)c)) out += c;
    else if (!out.empty() && out.back() != ' ') out += ' ';
  }
  if (!out.empty() && out.back() == ' ') out.pop_back();
  return out;
}

void usage() {
  fprintf(stderr,
          "k4align -i reads.f[aq][.gz] [-i more ...] [-u mates ...] -I index.sfx -o out.sam|out.bam [-z bgzf level=6] [-s subs/100bp=5] [-e 1|2] [-m 0..3] [-n maxNs=1]\n"
          "        [-U 0..4 PE mode] [-d minins=100] [-D maxins=1000] [-E] [-l minlen=50] [-L maxlen=500] [-r 0..5] [-R maxmulti=5] [-X] [-N] [-j unaligned.fa] [-J multialigned.fa] [-# every nth read] [-4 all @SQ up to n=10000] [-y trim5] [-Y trim3] [-H contaminants.fa flank contaminants trimmed off the read ends] [-Q 0|1|2 strand] [-M 0|1 all reads | -M3 --experimentid id --readsetid id: packed base alleles to -o, no SAM] [-c minchimeric%%] [-a microindel] [-A splicejunct] [-x flankexacts] [-k pcrwin 0..250] [-6 pcrprimersubs 0..5] [-5 lociconstraints.csv] [--chromexclude regex ...] [--chromeinclude regex ...] [--priorityregionfile regions.bed [-V | --nofiltpriority]] [-O stats.csv [-3 PE insert lengths per target to stats.csv.peinserts.csv]] [-8 siteprefs.csv [-9 ofs=-4]] [-p minsnpreads [-P qvalue=0.05] [-1 nonref%%=25] [-S snps.csv] [-7 centroids.csv] [-K markerlen 25..500 [--markerpolythres 0..0.5=0.333]]] [-S i/N] [-b MB per batch] [-B MB per upload=256] [-t io threads=8] [-Z] [-g 0..3 FASTQ qualities: Sanger | Illumina 1.3+ | Solexa | ignore=3] [-@ gpu=0] [-G gpu,gpu,... one rank per GPU]\n");
}

}  // namespace

// The C library's rand() as the reference binary sees it on Linux -- glibc's default TYPE_3 additive feedback generator,
// never seeded by kalign (seed 1): r[i] = r[i-3] + r[i-31] over 32-bit words, 310 values discarded, output = r[i] >> 1.
struct GlibcRand {
  uint32_t r[34];
  int k = 0;
  GlibcRand() {
    r[0] = 1;
    for (int i = 1; i < 31; i++) {
      int64_t v = (16807ll * (int32_t)r[i - 1]) % 2147483647ll;
      if (v < 0) v += 2147483647ll;
      r[i] = (uint32_t)v;
    }
    for (int i = 31; i < 34; i++) r[i] = r[i - 31];
    for (int i = 0; i < 310; i++) step();
  }
  uint32_t step() {  // ring of 34: r[k] holds x[i-34]; x[i] = x[i-3] + x[i-31]
    const uint32_t v = r[(k + 31) % 34] + r[(k + 3) % 34];
    r[k] = v;
    k = (k + 1) % 34;
    return v;
  }
  int next() { return (int)(step() >> 1); }
};
static GlibcRand draws;

static int run_multi_gpu(Opts& o, bool pe, int max_ml);

// <file cut at its last '.'> + suffix (CUtility::AppendFileNameSuffix): the side files of -O, -S and -M3
static std::string side_name(const std::string& path, const char* suffix) {
  std::string stem = path;
  for (size_t q = stem.size(); q > 0; q--) {
    if (stem[q - 1] == '.') { stem.resize(q - 1); break; }
    if (stem[q - 1] == '/' || stem[q - 1] == '\\') break;
  }
  return stem + suffix;
}
static bool ends_in(const std::string& name, const char* ext4) { return name.size() >= 4 && strcasecmp(name.c_str() + name.size() - 4, ext4) == 0; }
static bool create_empty(const std::string& path) {  // create / truncate
  FILE* fp = fopen(path.c_str(), "wb");
  if (fp) fclose(fp);
  return fp != nullptr;
}
// Every buffer to the file of its name.  All are tried; the first name that failed comes back (none: empty).  A `guarded` file
// that was created is one a failed run removes again.  big_by > 0: a buffer of 64 MB or more is written by that many threads side
// by side (the SNP coverage WIG of a genome at low coverage runs to gigabytes); everything else is written in order, pipes included.
struct NamedBuf { std::string name; const void* p; uint64_t n; bool guarded; };
static std::string write_files(const std::vector<NamedBuf>& files, std::vector<std::string>& made, int big_by) {
  std::string failed;
  for (const NamedBuf& f : files) {
    FILE* fp = fopen(f.name.c_str(), "wb");
    bool ok = fp != nullptr;
    if (ok && f.guarded) made.push_back(f.name);
    if (ok) ok = big_by > 0 && f.n >= (64u << 20) ? io_parallel<true>(fileno(fp), (uint8_t*)f.p, 0, f.n, big_by) : fwrite(f.p, 1, f.n, fp) == f.n;
    if (fp && fclose(fp) != 0) ok = false;
    if (!ok && failed.empty()) failed = f.name;
  }
  return failed;
}

// a device block into a file, 256 MB at a time; a write that failed shows in ferror(fp)
static int download(k4_index* ix, const void* d_src, uint64_t bytes, FILE* fp) {
  std::vector<char> piece((size_t)std::min<uint64_t>(bytes, 256ull << 20));
  for (uint64_t off = 0; off < bytes && !ferror(fp); off += piece.size()) {
    const uint64_t len = std::min<uint64_t>(piece.size(), bytes - off);
    const int rc = k4_copy_to_host(ix, piece.data(), (const char*)d_src + off, len);
    if (rc != K4_OK) return rc;
    fwrite(piece.data(), 1, len, fp);
  }
  return K4_OK;
}

// What a run holds.  However the run is left, they go in this order: the pipeline (its threads and pinned buffers); the outputs
// a failed run created (a SAM sized in advance and padded with NULs, a BAM without its end-of-file block: no artefact stays
// behind); the index -- closing it joins the library thread that may still be loading the .sfx, so main never returns and
// tears the runtime down under it.  The communicator goes behind the index, and only when this rank has met its peers at the
// closing barrier: a rank that fails must not enter a collective or a destroy its peers are not in (run_multi_gpu ends them).
struct RunHeld {
  k4_index* ix = nullptr;
  k4_pipeline* pl = nullptr;
  k4_comm* comm = nullptr;
  bool met_peers = false;
  std::vector<std::string> made;
  bool ok = false;
  void reset_pipeline() { if (pl) k4_pipeline_close(pl); pl = nullptr; }
  ~RunHeld() {
    reset_pipeline();
    for (const std::string& f : made) {
      struct stat sb;
      if (!ok && lstat(f.c_str(), &sb) == 0 && S_ISREG(sb.st_mode)) remove(f.c_str());  // (never a device node or /dev/stdout's link)
    }
    if (ix) k4_close(ix);
    if (comm && met_peers) k4_comm_close(comm);
  }
};

// One process, one GPU: the whole run, or rank o.rank of a -G run.  The state the steps of run_rank share; what it holds is the
// base, so the device blocks and tables below are gone before the index is.
struct Run : RunHeld {
  Opts& o;
  const bool pe, multi, chatty;  // (only rank 0 of a -G run reports)
  const int max_ml;
  const TimePoint t0 = now();
  TimePoint t_open;
  k4_info_t info;
  int mcl = 0, slides = 0;
  std::unique_ptr<k4_loci_constraint, void (*)(void*)> loci_tbl{nullptr, k4_free_host};  // -5
  int32_t n_loci = 0;
  std::vector<uint8_t> chrom_accept, hit_chrom;  // per sequence of the index: --chromexclude / --chromeinclude; has alignments
  k4_kalign_params kp;
  k4_pe_params pp;
  bool two_seg = false, pipelined = false, bam_out = false;
  k4_sam_stats tot;
  uint64_t n_under = 0, n_over = 0, n_units = 0, my_lines = 0;
  uint64_t n_contam[4] = {0, 0, 0, 0};  // -H: loaded reads with a 5' / 3' contaminant trim among PE1, among PE2
  double s_read = 0, s_parse = 0, s_align = 0, s_write = 0;
  k4_pipeline_view v;        // the pipelined modes: all reads of the run, aligned
  uint64_t pl_sam_bytes = 0;
  uint64_t stats_accepted = 0;  // -O: the accepted reads it counted (m_NARAccepted), which -3 goes by as well
  DevBlock keep_sam;         // -Z, -S i/N: the SAM body of the single batch stays on the device
  uint64_t keep_bytes = 0;
  std::vector<std::string> parts;  // -b: the batches' sorted bodies

  Run(Opts& opts, bool paired, int ml) : o(opts), pe(paired), multi(opts.n_ranks > 1 || opts.shared), chatty(opts.rank == 0), max_ml(ml) {
    memset(&tot, 0, sizeof(tot));
    memset(&v, 0, sizeof(v));
  }
  bool few_seqs() const { return info.n_entries <= (uint32_t)o.rpt_sq_thres; }  // m_MaxRptSAMSeqsThres, KAligner.cpp:5785-5821
  double index_secs() const { return std::max(secs(t0, t_open), k4_open_seconds(ix)); }

  // ---- the index: one GPU, or a rank of a -G run ---------------------------------------------------------------------------------
  // RCCL bring-up: rank 0 makes the communicator id, the others pick it up from the shared mapping; rank 0 reads the .sfx once;
  // sequence + suffix array reach the peers over xGMI; every rank builds its own tables.  K4ALIGN_FAULT=<rank>:<stage> is for the
  // tests of run_multi_gpu (see there)
  int open_rank_index() {
    int rc;
    const char* fault = getenv("K4ALIGN_FAULT");
    const int fault_rank = fault ? atoi(fault) : -1;
    const char* fault_stage = fault && strchr(fault, ':') ? strchr(fault, ':') + 1 : "";
    if (fault) {
      if (fault_rank == o.rank && strcmp(fault_stage, "start") == 0) { fprintf(stderr, "k4align: rank %d: injected fault at start\n", o.rank); return 3; }
      const char* peers = getenv("K4ALIGN_FAULT_PEERS");
      if (fault_rank != o.rank && peers && strcmp(peers, "block") == 0)
        for (;;) pause();  // what a rank blocked in a collective looks like to the parent
    }
    MultiShared* sh = o.shared;
    if (o.rank == 0) {
      if ((rc = k4_comm_unique_id(sh->id)) != K4_OK) { fprintf(stderr, "k4align: ncclGetUniqueId failed\n"); sh->failed = 1; return 2; }
      sh->id_ready = 1;
    } else
      while (!sh->id_ready.load()) { if (sh->failed.load()) return 2; usleep(1000); }
    if ((rc = k4_comm_init(o.gpu, o.rank, o.n_ranks, sh->id, &comm)) != K4_OK) { fprintf(stderr, "k4align: rank %d: RCCL communicator failed (%d)\n", o.rank, rc); sh->failed = 1; return 2; }
    rc = k4_comm_open_index(comm, o.rank == 0 ? o.sfx.c_str() : nullptr, 0, &ix);
    if (rc != K4_OK) { fprintf(stderr, "k4align: rank %d: index broadcast failed: %s (%d)\n", o.rank, k4_comm_last_error(comm), rc); sh->failed = 1; return 2; }
    if (fault_rank == o.rank && strcmp(fault_stage, "index") == 0) { fprintf(stderr, "k4align: rank %d: injected fault behind the index broadcast\n", o.rank); return 3; }
    return 0;
  }
  int open_index() {
    int rc;
    if (multi) {
      if ((rc = open_rank_index()) != 0) return rc;
    } else {
      // (the arrays load on a thread of the library while the reads are read: k4_open_wait in derive_params, or the pipeline's own)
      rc = k4_open_async(o.sfx.c_str(), o.gpu, 0, &ix);
      if (rc != K4_OK) { fprintf(stderr, "k4align: unable to load '%s': %s (%d)\n", o.sfx.c_str(), k4_global_error(), rc); return 2; }
    }
    k4_info(ix, &info);
    hit_chrom.assign(info.n_entries + 1, 0);
    if (o.q_method != 3) CK(k4_set_fastq_quality(ix, o.q_method));
    // SetMaxIter by sensitivity, KAligner.cpp:373-388
    k4_set_max_iter(ix, o.pmode == 2 ? 20000 : o.pmode == 1 ? 10000 : o.pmode == 0 ? 5000 : 2500);
    mcl = k4_min_core_len(ix, o.pmode, &slides);
    if (chatty)
      fprintf(stderr, "k4align: index '%s' %u sequences, %llu bp; minimum core size %dbp%s\n", info.dataset, info.n_entries,
              (unsigned long long)info.tot_seqs_len, mcl, multi ? " (read once, sent to the other GPUs over xGMI)" : "");
    t_open = now();
    return 0;
  }
  // -5 and --chromexclude / --chromeinclude, checked against the index's sequences before any read is loaded (KAligner.cpp:4619-4628)
  int load_constraints() {
    int rc;
    if (!o.loci_file.empty()) {
      k4_loci_constraint* t = nullptr;
      if ((rc = k4_load_loci_constraints(ix, o.loci_file.c_str(), &t, &n_loci, nullptr)) != K4_OK) {
        fprintf(stderr, "k4align: %s (%d)\n", k4_last_error(ix), rc);
        return rc == K4_ERR_OPEN_FILE ? 2 : 1;
      }
      loci_tbl.reset(t);
      if (chatty) fprintf(stderr, "k4align: %d loci base constraints loaded from '%s'\n", (int)n_loci, o.loci_file.c_str());
    }
    if (!o.chrom_excl.empty() || !o.chrom_incl.empty()) {  // one decision per sequence of the index, made here once
      std::vector<const char*> inc, exc;
      for (const std::string& q : o.chrom_incl) inc.push_back(q.c_str());
      for (const std::string& q : o.chrom_excl) exc.push_back(q.c_str());
      chrom_accept.assign((size_t)info.n_entries + 1, 0);
      if ((rc = k4_chrom_accept_mask(ix, (int32_t)inc.size(), inc.data(), (int32_t)exc.size(), exc.data(), chrom_accept.data())) != K4_OK) {
        fprintf(stderr, "k4align: %s (%d)\n", k4_last_error(ix), rc);
        return 1;
      }
    }
    if (!o.priority_file.empty()) {  // the BED file's features on the index's sequences (KAligner.cpp:311-330); names the index lacks are dropped
      std::vector<K4BedFeature> feats;
      if (k4_read_bed_features(o.priority_file.c_str(), &feats) != 0) {
        fprintf(stderr, "k4align: Unable to open high priority regions BED file '%s'\n", o.priority_file.c_str());
        return 2;
      }
      std::unordered_map<std::string, int> names;  // lower-cased BED name -> its number; the features by that number
      std::vector<std::vector<size_t>> feats_of;
      for (size_t k = 0; k < feats.size(); k++) {
        const auto it = names.emplace(k4_bed_lower(feats[k].chrom.c_str()), (int)feats_of.size());
        if (it.second) feats_of.emplace_back();
        feats_of[(size_t)it.first->second].push_back(k);
      }
      std::vector<uint32_t> ids, starts, ends;
      for (uint32_t c = 1; c <= info.n_entries; c++) {
        k4_entry e;
        if (k4_get_entry(ix, c, &e) != K4_OK) continue;
        const int q = k4_bed_locate_chrom(names, e.name);
        if (q < 0) continue;
        for (const size_t k : feats_of[(size_t)q]) { ids.push_back(c); starts.push_back(feats[k].start); ends.push_back(feats[k].end); }
      }
      CK(k4_set_priority_regions(ix, (int64_t)ids.size(), ids.data(), starts.data(), ends.data()));
      if (chatty) fprintf(stderr, "k4align: High priority regions BED file '%s' loaded: %zu features on sequences of the index\n", o.priority_file.c_str(), ids.size());
    }
    return 0;
  }
  // the combinations that need the run's mode, the parameters of the alignment, and which input and output path this run takes
  int derive_params() {
    if ((o.ml_mode == 3 || o.ml_mode == 4) && (o.batch_mb > 0 || o.n_shards > 1)) {
      fprintf(stderr, "k4align: -r3 / -r4 cluster over all reads of the run; they cannot be combined with -b or -S\n");
      return 1;
    }
    if (o.batch_mb > 0 && o.n_shards > 1) { fprintf(stderr, "k4align: -S slices the whole input; it cannot be combined with -b\n"); return 1; }
    if ((o.micro_indel || o.splice_junct) && (o.batch_mb > 0 || o.n_shards > 1)) {
      fprintf(stderr, "k4align: -a / -A drop junctions no second read of the RUN supports; they cannot be combined with -b or -S\n");
      return 1;
    }
    // -6: the reads are aligned with m_InitalAlignSubs (KAligner.cpp:245-248, :504, :607); everything else keeps the user's -s
    const int align_subs = o.primer_subs > 0 ? std::min(o.max_subs + o.primer_subs, 15) : o.max_subs;
    kp = {align_subs, o.min_edit, o.max_ns, o.pmode, o.align_strand /* K4_STRAND_*: the same codes as eALStrand */, max_ml,
          o.ml_mode == 5 ? (o.best ? 4 : o.clamp ? 3 : 2) : o.ml_mode == 2 ? 2 : o.ml_mode != 0 ? 1 : 0,
          mcl, slides, o.min_chimeric, o.micro_indel, o.splice_junct};
    two_seg = o.micro_indel > 0 || o.splice_junct > 0;
    pp = {o.pe_mode, o.pair_min, o.pair_max, o.pair_strand};
    // default: the overlapped pipeline (k4_pipeline_*): reader threads -> pinned ring -> copy stream || parse + align on the
    // compute stream; one global sort + SAM body at the end, handed out while its next pieces come down.
    // -b <MB>: bounded memory, coordinate-sorted parts merged on the host; -S i/N: one slice of the reads (one process per GPU)
    pipelined = o.batch_mb <= 0 && o.n_shards == 1 && !o.legacy;
    bam_out = o.rank_bam || ends_in(o.out, ".bam");  // "-o x.bam": BGZF compressed BAM, any other extension SAM (KAlignerCL.cpp:857-866)
    int rc;
    if (!pipelined && !multi && (rc = k4_open_wait(ix)) != K4_OK) { fprintf(stderr, "k4align: unable to load '%s': %s (%d)\n", o.sfx.c_str(), k4_global_error(), rc); return 2; }
    if (bam_out && (!pipelined || (multi && !o.rank_bam))) { fprintf(stderr, "k4align: BAM output is written by the pipelined modes (not with -b, -S, -Z)\n"); return 3; }
    return 0;
  }

  // ---- the input, pipelined ------------------------------------------------------------------------------------------------------
  int open_pipeline() {
    for (const std::vector<std::string>* fs : {&o.in1, &o.in2})
      for (const std::string& q : *fs) {
        FILE* t = fopen(q.c_str(), "rb");
        if (!t) { fprintf(stderr, "k4align: unable to open '%s'\n", q.c_str()); return 2; }
        fclose(t);
      }
    k4_pipeline_params pp2;
    memset(&pp2, 0, sizeof(pp2));
    pp2.paired = pe ? 1 : 0; pp2.kp = kp; pp2.pe = pp; pp2.min_len = o.min_len; pp2.max_len = o.max_len;
    pp2.chunk_bytes = (uint64_t)o.chunk_mb << 20;
    for (int e = 0; e < (pe ? 2 : 1); e++) {
      bool plain = true;
      uint64_t tot_sz = 0;
      for (const std::string& q : e ? o.in2 : o.in1) { plain &= !is_gzip(q); tot_sz += file_size(q) + 1; }
      pp2.expect_text_bytes[e] = plain ? tot_sz : 0;
    }
    if (!o.stats_file.empty()) {  // created / truncated before the reads are loaded (KAligner.cpp:4705-4730); a failed run leaves none of the three
      if (!create_empty(o.stats_file)) { fprintf(stderr, "k4align: unable to create/truncate output stats file '%s'\n", o.stats_file.c_str()); return 5; }
      made.push_back(o.stats_file);
      made.push_back(side_name(o.stats_file, ".AlignCntsDist.csv"));
      if (pe) made.push_back(side_name(o.stats_file, ".GlobalPEInsertDist.csv"));
      if (o.pe_insert_dist) {  // (KAligner.cpp:4731-4752)
        const std::string fn = o.stats_file + ".peinserts.csv";
        if (!create_empty(fn)) { fprintf(stderr, "k4align: unable to create/truncate PE insert length distributions file '%s'\n", fn.c_str()); return 5; }
        made.push_back(fn);
      }
      CK(k4_align_stats_collect(ix, 1));
    }
    if (!o.site_file.empty()) {  // created / truncated with the other outputs (KAligner.cpp:4471-4491); it stays empty when no read is accepted
      if (!create_empty(o.site_file)) { fprintf(stderr, "k4align: unable to create/truncate site preferencing file '%s'\n", o.site_file.c_str()); return 5; }
      made.push_back(o.site_file);
    }
    CK(k4_pipeline_open(ix, &pp2, &pl));
    CK(k4_pipeline_set_trims(pl, o.trim5, o.trim3));
    CK(k4_pipeline_set_sampling(pl, o.sample_nth));
    if (o.contam_tbl) CK(k4_pipeline_set_contaminants(pl, o.contam_tbl, o.n_contam_tbl));
    return 0;
  }
  // -G over uncompressed files: reads are independent units, rank r aligns the r-th contiguous slice of the records (pairs stay
  // together).  Rank 0 finds the slice boundaries (one pass over the files), every rank then reads only its own byte range
  int rank_ranges(std::vector<FileRange> fr[2]) {
    MultiShared* sh = o.shared;
    if (o.rank == 0) {
      uint64_t R = 0, R2 = 0;
      std::vector<uint64_t> counts;
      std::string why;
      bool ok = slice_files(o.in1, o.n_ranks, counts, false, sh->slice_off[0], &R, o.io_threads, &why);
      if (ok && pe) ok = o.in2.size() == o.in1.size() ? slice_files(o.in2, o.n_ranks, counts, true, sh->slice_off[1], &R2, o.io_threads, &why)
                                                      : (why = "as many -u files as -i files are needed", false);
      if (!ok) { fprintf(stderr, "k4align: unable to cut the reads into slices: %s\n", why.c_str()); sh->failed = 1; return 2; }
      sh->n_records = R;
      sh->slices_ready = 1;
    } else
      while (!sh->slices_ready.load()) { if (sh->failed.load()) return 2; usleep(1000); }
    for (int e = 0; e < (pe ? 2 : 1); e++) {
      const std::vector<std::string>& fl = e ? o.in2 : o.in1;
      for (size_t f = 0; f < fl.size(); f++)
        fr[e].push_back(FileRange{fl[f], sh->slice_off[e][f][o.rank], sh->slice_off[e][f][o.rank + 1], file_size(fl[f])});
    }
    return 0;
  }
  // one reader per end fills the pipeline (the second end on a thread of its own); then all reads of the run are aligned
  int feed_pipeline() {
    bool any_gz = false;  // a -G run: no byte offsets into a compressed stream, record blocks are dealt to the ranks
    for (const std::string& q : o.in1) any_gz |= is_gzip(q);
    for (const std::string& q : o.in2) any_gz |= is_gzip(q);
    std::vector<FileRange> fr[2];
    auto tr = now();
    int rc;
    if (multi && !any_gz && (rc = rank_ranges(fr)) != 0) return rc;
    int rc_end[2] = {K4_OK, K4_OK};
    double rd[2] = {0, 0};
    auto feed = [&](int e) {
      const std::vector<std::string>& files = e ? o.in2 : o.in1;
      rc_end[e] = !multi  ? feed_end(pl, e, files, o.io_threads, &rd[e])
                  : any_gz ? feed_dealt(pl, e, files, o.rank, o.n_ranks, &rd[e])
                           : feed_ranges(pl, e, fr[e], o.io_threads, &rd[e]);
    };
    std::thread t2;
    if (pe) t2 = std::thread(feed, 1);
    feed(0);
    if (pe) t2.join();
    s_read = std::max(rd[0], rd[1]);
    for (int e = 0; e < 2; e++)
      if (rc_end[e] != K4_OK) { fprintf(stderr, "k4align: error reading the input (%d): %s\n", rc_end[e], k4_last_error(ix)); return 2; }
    CK(k4_pipeline_wait_aligned(pl, &v));
    s_parse = secs(tr, now()) - s_read;  // what the device side added behind the reading
    return 0;
  }

  // ---- the stages between alignment and report, over ALL reads of the run (CKAligner::Align, KAligner.cpp:615-686) -----------------
  int global_stages(int64_t n, uint32_t max_len, void* d_rr, void* d_hits, void* d_seg2, void* d_pe, void* d_reads, void* d_offs, void* d_lens) {
    if (n <= 0 || max_len == 0) return K4_OK;
    if (!pe) {
      if (o.ml_mode == 3 || o.ml_mode == 4) {  // AssignMultiMatches (KAligner.cpp:5092): clusters over all reads of the run
        int64_t n_assigned = 0;
        CK(k4_assign_multi_dev(ix, o.ml_mode, (int32_t)max_len, n, max_ml, d_rr, d_hits, &n_assigned, nullptr));
        fprintf(stderr, "k4align: %lld multi-aligned reads assigned to one locus by clustering\n", (long long)n_assigned);
      }
      if (o.ml_mode == 2) {
        // eMLrand (KAligner.cpp:9945-9962): rand() once per read within the instance limit, in load order -- what the
        // reference does when it runs one thread (with more its draws depend on thread timing).  The draws are a private
        // restatement of the C library's generator: other code in this process (the HIP runtime) may call rand() too
        std::vector<k4_read_result> rr((size_t)n);
        std::vector<uint32_t> choice((size_t)n, 0);
        CK(k4_copy_to_host(ix, rr.data(), d_rr, (uint64_t)n * sizeof(k4_read_result)));
        for (int64_t i = 0; i < n; i++)
          if (rr[i].nar == K4_NAR_ACCEPTED && rr[i].num_hits >= 1) choice[i] = (uint32_t)(draws.next() % rr[i].num_hits);
        DevBlock d_choice;
        CK(alloc_dev(ix, (uint64_t)n * 4, d_choice));
        CK(k4_copy_to_device(ix, d_choice.get(), choice.data(), (uint64_t)n * 4));
        CK(k4_select_hits_dev(ix, n, max_ml, d_rr, d_hits, d_choice.get(), nullptr));
      }
    }
    int64_t cnt = 0;
    if (n_loci > 0) {  // IdentifyConstraintViolations: behind ProcessPairedEnds / AssignMultiMatches, in front of ReducePCRduplicates (KAligner.cpp:628)
      CK(k4_filter_loci_constraints_dev(ix, loci_tbl.get(), n_loci, pe ? 1 : 0, n, max_ml, d_rr, d_hits, d_seg2, d_pe, d_reads, d_offs, d_lens, &cnt,
                                        nullptr));
      fprintf(stderr, "k4align: %lld loci base constraint violations\n", (long long)cnt);
    }
    if (!pe && o.pcr_win >= 0) {  // ReducePCRduplicates, behind AssignMultiMatches and before the filters (KAligner.cpp:628-640)
      CK(k4_reduce_pcr_dups_dev(ix, o.pcr_win, n, max_ml, d_rr, d_hits, &cnt, nullptr));
      fprintf(stderr, "k4align: %lld potential PCR artefact reads removed\n", (long long)cnt);
    }
    if (o.primer_subs > 0) {  // PCR5PrimerCorrect, behind ReducePCRduplicates and in front of AutoTrimFlanks, SE and PE (KAligner.cpp:642-651)
      int64_t c3[3] = {0, 0, 0};
      CK(k4_pcr5_primer_correct_dev(ix, o.max_subs, 12, pe ? 1 : 0, pe ? 2 * n : n, max_ml, pe ? d_pe : d_rr, d_hits, d_reads, d_offs, d_lens, c3, nullptr));
      fprintf(stderr, "k4align: PCR 5' primer correction: %lld reads with %lld bases corrected, %lld reads with excessive substitutions rejected\n",
              (long long)c3[0], (long long)c3[1], (long long)c3[2]);
    }
    // the filters, in CKAligner::Align's order (KAligner.cpp:653-686)
    if (o.min_flank_exacts > 0) {
      CK(k4_auto_trim_flanks_dev(ix, o.min_flank_exacts, pe ? 1 : 0, pe ? 2 * n : n, max_ml, pe ? d_pe : d_rr, d_hits, d_reads, d_offs,
                                 d_lens, &cnt, nullptr));
      fprintf(stderr, "k4align: flank autotrim to %d exact bases: %lld aligned reads removed\n", o.min_flank_exacts, (long long)cnt);
    }
    if (!pe && o.splice_junct > 0) {
      CK(k4_remove_orphan_juncts_dev(ix, K4_EXT_SPLICE, n, max_ml, d_rr, d_hits, d_seg2, &cnt, nullptr));
      fprintf(stderr, "k4align: %lld orphan splice junction reads removed\n", (long long)cnt);
    }
    if (!pe && o.micro_indel > 0) {
      CK(k4_remove_orphan_juncts_dev(ix, K4_EXT_INDEL, n, max_ml, d_rr, d_hits, d_seg2, &cnt, nullptr));
      fprintf(stderr, "k4align: %lld orphan microInDel reads removed\n", (long long)cnt);
    }
    if (!chrom_accept.empty()) {  // FiltByChroms: behind the autotrim and the orphan filters, in front of every report (KAligner.cpp:693)
      DevBlock d_accept;
      CK(alloc_dev(ix, chrom_accept.size(), d_accept));
      CK(k4_copy_to_device(ix, d_accept.get(), chrom_accept.data(), chrom_accept.size()));
      CK(k4_filter_chroms_dev(ix, d_accept.get(), pe ? 1 : 0, pe ? 2 * n : n, max_ml, pe ? d_pe : d_rr, d_hits, &cnt, nullptr));
      fprintf(stderr, "k4align: %lld matches removed by chromosome filtering\n", (long long)cnt);
    }
    if (!o.priority_file.empty() && !o.no_filt_priority) {  // FiltByPriorityRegions: directly behind FiltByChroms (KAligner.cpp:705)
      CK(k4_filter_priority_regions_dev(ix, pe ? 1 : 0, pe ? 2 * n : n, max_ml, pe ? d_pe : d_rr, d_hits, pe ? nullptr : d_seg2, &cnt, nullptr));
      fprintf(stderr, "k4align: %lld matches removed by priority region filtering\n", (long long)cnt);
    }
    return K4_OK;
  }

  // ---- the reports of the pipelined modes, in front of the alignments' own ---------------------------------------------------------
  int write_unaligned() {  // ReportNoneAligned / ReportMultiAlign (KAligner.cpp:709-733)
    for (int which = 0; which < 2; which++) {
      const std::string& fn = which ? o.multi_file : o.none_file;
      if (fn.empty()) continue;
      char* txt = nullptr;
      uint64_t nb = 0, nl = 0;
      CK(k4_unaligned_fasta_dev(ix, pe ? 1 : 0, v.n_units, v.d_rr, v.d_pe, v.d_reads, v.d_offs, v.d_lens, &v.names, which, &txt, &nb, &nl, nullptr));
      const std::string failed = write_files({{fn, txt, nb, false}}, made, 0);
      k4_free_host(txt);
      if (!failed.empty()) { fprintf(stderr, "k4align: unable to write %s\n", fn.c_str()); return 5; }
      if (chatty) fprintf(stderr, "k4align: %llu %s reads written to %s\n", (unsigned long long)nl, which ? "multi-aligned" : "unalignable", fn.c_str());
    }
    return 0;
  }
  int write_pba() {  // genpba: ProcessSNPs in PBA mode is the report (KAligner.cpp:741-790); no SAM is written
    auto ts = now();
    k4_pba_files pf;
    CK(k4_pba_run_dev(ix, pe ? 1 : 0, v.n_units, v.d_rr, v.d_hits, v.max_ml, v.d_pe, v.d_reads, v.d_offs, v.d_lens, o.experiment_id.c_str(),
                      o.readset_id.c_str(), &pf, nullptr));
    const std::string wig = side_name(o.out, ".covsegs.wig");  // (KAligner.cpp:4341)
    const std::string failed = write_files({{o.out, pf.pba, pf.pba_bytes, true}, {wig, pf.wig, pf.wig_bytes, true}}, made, 0);
    k4_free_host(pf.pba); k4_free_host(pf.wig);
    if (!failed.empty()) { fprintf(stderr, "k4align: unable to write %s\n", failed.c_str()); return 5; }
    if (chatty) fprintf(stderr, "k4align: packed base alleles of %llu sequences (%llu bytes) written to %s, coverage to %s in %.2fs\n",
                        (unsigned long long)pf.n_chroms, (unsigned long long)pf.pba_bytes, o.out.c_str(), wig.c_str(), secs(ts, now()));
    ok = true;
    return 0;
  }
  int write_snps() {  // ProcessSNPs (KAligner.cpp:768-790 calls it behind the alignment report): the SNP file and its side files
    auto ts = now();
    const bool vcf = ends_in(o.snp_file, ".vcf");  // VCF instead of the CSV (KAligner.cpp:186-187)
    k4_snp_files sf;
    k4_snp_files2 sf2;
    memset(&sf2, 0, sizeof(sf2));
    const bool more = o.marker_len != 0 || !o.cent_file.empty();  // the marker and centroid files out of the same counts
    if (more) {
      k4_snp_opts so;
      so.marker_len = o.marker_len; so.want_centroids = o.cent_file.empty() ? 0 : 1; so.marker_poly_thres = o.marker_poly_thres;
      CK(k4_snp_run2_dev(ix, vcf ? 1 : 0, pe ? 1 : 0, v.n_units, v.d_rr, v.d_hits, v.max_ml, v.d_pe, v.d_reads, v.d_offs, v.d_lens, o.min_snp_reads,
                         o.qvalue, o.snp_nonref_pcnt, &so, &sf2, nullptr));
      sf = sf2.files;
    } else
      CK(k4_snp_run_dev(ix, vcf ? 1 : 0, pe ? 1 : 0, v.n_units, v.d_rr, v.d_hits, v.max_ml, v.d_pe, v.d_reads, v.d_offs, v.d_lens, o.min_snp_reads,
                        o.qvalue, o.snp_nonref_pcnt, &sf, nullptr));
    // (the side files: KAligner.cpp:4512, 4553-4554)
    std::vector<NamedBuf> files = {{side_name(o.snp_file, ".covsegs.wig"), sf.wig, sf.wig_bytes, false},
                                   {side_name(o.snp_file, ".disnp.csv"), sf.disnp, sf.disnp_bytes, false},
                                   {side_name(o.snp_file, ".trisnp.csv"), sf.trisnp, sf.trisnp_bytes, false},
                                   {o.snp_file, sf.snp, sf.snp_bytes, false}};
    if (o.marker_len) files.push_back({o.snp_file + ".markers", sf2.markers, sf2.markers_bytes, true});  // (the name is appended, KAlignerCL.cpp:957-959)
    if (!o.cent_file.empty()) files.push_back({o.cent_file, sf2.centroids, sf2.centroids_bytes, true});
    const std::string failed = write_files(files, made, std::max(o.io_threads, 1));
    k4_free_host(sf.snp); k4_free_host(sf.wig); k4_free_host(sf.disnp); k4_free_host(sf.trisnp);
    k4_free_host(sf2.markers); k4_free_host(sf2.centroids);
    if (!failed.empty()) { fprintf(stderr, "k4align: unable to write %s\n", failed.c_str()); return 5; }
    if (chatty) fprintf(stderr, "k4align: SNP processing completed with %llu putative SNPs discovered, written to %s in %.2fs\n",
                        (unsigned long long)sf.n_snps, o.snp_file.c_str(), secs(ts, now()));
    if (chatty && o.marker_len) fprintf(stderr, "k4align: %llu marker sequences of %d bases written to %s.markers\n", (unsigned long long)sf2.n_markers,
                                        o.marker_len, o.snp_file.c_str());
    if (chatty && !o.cent_file.empty()) fprintf(stderr, "k4align: SNP centroid distribution written to %s\n", o.cent_file.c_str());
    return 0;
  }
  int write_align_stats() {  // -O, behind every stage that can still drop a read: the counted reads are the reported ones
    auto ts = now();
    k4_align_stats as;
    CK(k4_pipeline_align_stats(pl, &as));
    const uint64_t loaded = (uint64_t)(pe ? 2 : 1) * ((uint64_t)v.n_units - v.n_under - v.n_over);
    if (o.splice_junct > 0) {
      // with -A and SAM output the reference has its splice junction file open (KAligner.cpp:4446), so WriteReadHits runs in front
      // of WriteBAMReadHits (:745-757) and calls WriteSubDist for every read too (:6835): those counts come out doubled
      for (uint64_t q = 0; q < 4ull * as.len_stride; q++) { as.q_insts[q] *= 2; as.q_subs[q] *= 2; }
      for (uint64_t q = 0; q <= as.len_stride; q++) as.m_sub[q] *= 2;
    }
    const int rc = k4_write_align_stats(ix, &as, loaded, o.ml_mode, max_ml, pe ? 1 : 0, o.stats_file.c_str());
    stats_accepted = as.n_accepted;
    k4_free_align_stats(&as);
    if (rc != K4_OK) { fprintf(stderr, "k4align: %s\n", k4_last_error(ix)); return 5; }
    if (chatty) fprintf(stderr, "k4align: alignment statistics written to %s in %.2fs\n", o.stats_file.c_str(), secs(ts, now()));
    return 0;
  }
  int write_pe_insert_dist() {  // -3 (PE with -O): ReportPEInsertLenDist walks the reads the writer reports (KAligner.cpp:771)
    auto ts = now();
    const std::string fn = o.stats_file + ".peinserts.csv";  // (:205-215: appended to the whole name)
    k4_pe_insert_dist pd;
    CK(k4_pipeline_pe_insert_dist(pl, &pd));
    const uint32_t n_rows = pd.n_rows;
    const int rc = k4_write_pe_insert_dist(ix, &pd, stats_accepted, fn.c_str());
    k4_free_pe_insert_dist(&pd);
    if (rc != K4_OK) { fprintf(stderr, "k4align: %s\n", k4_last_error(ix)); return 5; }
    if (chatty) fprintf(stderr, "k4align: PE insert lengths of %u target sequences written to %s in %.2fs\n", n_rows, fn.c_str(), secs(ts, now()));
    return 0;
  }
  int write_site_prefs() {  // -8: ProcessSiteProbabilites runs in front of the writer (KAligner.cpp:743), over the reads it will report
    auto ts = now();
    k4_site_prefs sp;
    CK(k4_pipeline_site_prefs(pl, o.site_ofs, &sp));
    const int rc = k4_write_site_prefs(&sp, o.site_file.c_str());
    k4_free_site_prefs(&sp);
    if (rc != K4_OK) { fprintf(stderr, "k4align: %s\n", k4_global_error()); return 5; }
    if (chatty) fprintf(stderr, "k4align: start site octamer preferences written to %s in %.2fs\n", o.site_file.c_str(), secs(ts, now()));
    return 0;
  }
  int format_records() {  // the global sort and the SAM body / BAM records of all reads, on the device
    // (a rank of a -G run numbers every sequence: the parent renumbers when it knows which ones any rank has hit)
    const int bam_all_sq = (few_seqs() || o.rank_bam) ? 1 : 0;
    if (bam_out && o.fmode == 1) CK(k4_pipeline_format_bam_all(pl, bam_all_sq, &tot, hit_chrom.data(), &pl_sam_bytes));
    else if (bam_out) CK(k4_pipeline_format_bam(pl, bam_all_sq, &tot, hit_chrom.data(), &pl_sam_bytes));
    else if (o.fmode == 1) CK(k4_pipeline_format_all(pl, &tot, hit_chrom.data(), &pl_sam_bytes));
    else CK(k4_pipeline_format(pl, &tot, hit_chrom.data(), &pl_sam_bytes));
    n_under = v.n_under; n_over = v.n_over; n_units = (uint64_t)v.n_units;
    return 0;
  }

  // ---- the input, streamed (-b) or whole (-Z, -S i/N) -------------------------------------------------------------------------------
  // One batch: text holding whole records (the last one possibly cut when more text follows) -> records -> alignments ->
  // SAM body.  The body goes to `body` (a part file) or, for the single batch of the whole-input mode, stays on the device.
  int run_batch(const uint8_t* t1, uint64_t T1, int fin1, const uint8_t* t2, uint64_t T2, int fin2, FILE* body, uint64_t* used1, uint64_t* used2) {
    *used1 = *used2 = 0;
    auto ta = now();
    DevBlock d_reads, d_offs, d_lens, d_rr, d_hits, d_pe, d_seg2;
    CK(alloc_dev(ix, T1 + T2 + 64, d_reads));
    Parsed p1, p2;
    CK(load_reads(ix, t1, T1, fin1, 0, d_reads.get(), 0, p1, used1));
    if (pe) {
      CK(load_reads(ix, t2, T2, fin2, (int64_t)std::max<uint64_t>(p1.n, 1), d_reads.get(), p1.bases, p2, used2));
      if (p2.n < p1.n) {  // this portion of the mates' file holds fewer records: keep the pairs both files delivered
        if (fin2 && fin1) { fprintf(stderr, "k4align: fewer PE2 than PE1 reads\n"); return 3; }
        const int64_t n2 = (int64_t)p2.n;
        p1 = Parsed();
        p2 = Parsed();
        if (n2 == 0) { *used1 = *used2 = 0; return K4_OK; }
        CK(load_reads(ix, t1, T1, fin1, n2, d_reads.get(), 0, p1, used1));
        CK(load_reads(ix, t2, T2, fin2, n2, d_reads.get(), p1.bases, p2, used2));
      }
    }
    // -S i/N: reads (pairs) are independent units; every process parses the whole input -- that is cheap
    // on the device -- and keeps its contiguous slice, so that the shards' SAM files merge back into load order (k4merge)
    const int64_t r0 = (int64_t)p1.n * o.shard / o.n_shards, r1 = (int64_t)p1.n * (o.shard + 1) / o.n_shards;
    auto from_r0 = [r0](const DevBlock& b, int width) -> void* { return b ? (uint8_t*)b.get() + width * r0 : nullptr; };
    const int64_t n = r1 - r0;
    const int64_t n_reads = pe ? 2 * n : n;
    uint64_t under = 0, over = 0;
    uint32_t max_len = 0;
    CK(alloc_dev(ix, (uint64_t)(n_reads + 1) * 8, d_offs));
    CK(alloc_dev(ix, (uint64_t)(n_reads + 1) * 4, d_lens));
    if (!o.contam_tbl)
      CK(k4_prepare_reads_trim_dev(ix, pe ? 1 : 0, n, o.min_len, o.max_len, o.trim5, o.trim3, 1, 0, from_r0(p1.offs, 8), from_r0(p1.lens, 4),
                                   from_r0(p2.offs, 8), from_r0(p2.lens, 4), 0, d_offs.get(), d_lens.get(), &under, &over, &max_len, nullptr));
    else {  // -H: the same ingest calls as the pipeline's (every batch, every slice: the stage is per read)
      DevBlock d_c5, d_c3;
      uint64_t nc[4];
      CK(alloc_dev(ix, (uint64_t)n_reads + 1, d_c5));
      CK(alloc_dev(ix, (uint64_t)n_reads + 1, d_c3));
      CK(k4_contam_trims_dev(ix, o.contam_tbl, o.n_contam_tbl, pe ? 1 : 0, n, o.trim5, o.trim3, 1, 0, d_reads.get(), from_r0(p1.offs, 8), from_r0(p1.lens, 4),
                             from_r0(p2.offs, 8), from_r0(p2.lens, 4), 0, d_c5.get(), d_c3.get(), nullptr, nullptr));
      CK(k4_prepare_reads_contam_dev(ix, pe ? 1 : 0, n, o.min_len, o.max_len, o.trim5, o.trim3, 1, 0, from_r0(p1.offs, 8), from_r0(p1.lens, 4),
                                     from_r0(p2.offs, 8), from_r0(p2.lens, 4), 0, d_c5.get(), d_c3.get(), d_offs.get(), d_lens.get(), &under, &over,
                                     &max_len, nc, nullptr));
      for (int k = 0; k < 4; k++) n_contam[k] += nc[k];
    }
    auto tb = now();
    // ---- align (ProcCoredApprox / ProcessPairedEnds), the global stages, the SAM body on the device (k4_format_sam_dev) ----------
    k4_sam_names nm;
    memset(&nm, 0, sizeof(nm));
    nm.d_text[0] = p1.text.get(); nm.d_name_off[0] = from_r0(p1.noff, 8); nm.d_name_len[0] = from_r0(p1.nlen, 4);
    nm.d_text[1] = p2.text.get(); nm.d_name_off[1] = from_r0(p2.noff, 8); nm.d_name_len[1] = from_r0(p2.nlen, 4);
    void* d_sam = nullptr;
    uint64_t sam_bytes = 0;
    k4_sam_stats stt;
    memset(&stt, 0, sizeof(stt));
    std::vector<uint8_t> hc(info.n_entries + 1, 0);
    if (n > 0 && max_len > 0) {
      if (!pe) {
        CK(alloc_dev(ix, (uint64_t)n * sizeof(k4_read_result), d_rr));
        CK(alloc_dev(ix, (uint64_t)n * max_ml * sizeof(k4_hit), d_hits));
        if (two_seg) CK(alloc_dev(ix, (uint64_t)n * sizeof(k4_seg2), d_seg2));
        CK(k4_reserve(ix, n, (int32_t)max_len, max_ml));
        CK(k4_kalign_ext_batch_dev(ix, &kp, n, (int32_t)max_len, d_reads.get(), d_offs.get(), d_lens.get(), d_rr.get(), d_hits.get(), d_seg2.get(), nullptr));
      } else {
        CK(alloc_dev(ix, (uint64_t)2 * n * sizeof(k4_pe_read), d_pe));
        CK(k4_kalign_pe_batch_dev(ix, &kp, &pp, n, (int32_t)max_len, d_reads.get(), d_offs.get(), d_lens.get(), d_pe.get(), nullptr));
      }
      const int rc = global_stages(n, max_len, d_rr.get(), d_hits.get(), d_seg2.get(), d_pe.get(), d_reads.get(), d_offs.get(), d_lens.get());
      if (rc != K4_OK) return rc;
      CK(k4_format_sam_ext_dev(ix, pe ? 1 : 0, n, d_rr.get(), d_hits.get(), max_ml, d_pe.get(), d_seg2.get(), d_reads.get(), d_offs.get(), d_lens.get(), &nm,
                               &d_sam, &sam_bytes, &stt, hc.data(), nullptr));
    }
    keep_sam.reset(d_sam);
    keep_bytes = sam_bytes;
    auto tc = now();
    for (int k = 0; k < 20; k++) tot.nar[k] += stt.nar[k];
    tot.plus += stt.plus; tot.minus += stt.minus; tot.n_lines += stt.n_lines;
    for (size_t c = 0; c < hc.size(); c++) hit_chrom[c] |= hc[c];
    n_under += under; n_over += over; n_units += (uint64_t)n;
    if (body) {
      CK(download(ix, d_sam, sam_bytes, body));
      if (ferror(body)) { fprintf(stderr, "k4align: write failed\n"); return 5; }
      keep_sam.reset();
    }
    s_parse += secs(ta, tb); s_align += secs(tb, tc); s_write += secs(tc, now());
    return K4_OK;
  }
  int stream_batches() {
    Stream f1, f2;
    if (!f1.open(o.in1) || (pe && !f2.open(o.in2))) { fprintf(stderr, "k4align: unable to open reads\n"); return 2; }
    const bool whole = o.batch_mb <= 0;
    const uint64_t want0 = whole ? UINT64_MAX : std::max<uint64_t>((uint64_t)(o.batch_mb * 1048576.0), 4096);
    uint64_t want = want0;
    for (;;) {
      auto tr = now();
      if (!f1.fill(want) || (pe && !f2.fill(want))) { fprintf(stderr, "k4align: error reading the input\n"); return 2; }
      s_read += secs(tr, now());
      if (f1.buf.empty()) break;
      FILE* body = nullptr;
      if (!whole) {
        parts.push_back(o.out + ".part" + std::to_string(parts.size()));
        body = fopen(parts.back().c_str(), "wb");
        if (!body) { fprintf(stderr, "k4align: unable to create %s\n", parts.back().c_str()); return 5; }
      }
      uint64_t u1 = 0, u2 = 0;
      const int rc = run_batch(f1.buf.data(), f1.buf.size(), f1.eof, f2.buf.data(), f2.buf.size(), f2.eof, body, &u1, &u2);
      if (body) fclose(body);
      if (rc != K4_OK) return rc;
      if (u1 == 0) {  // not one whole record (pair) in this much text
        if (!whole) { remove(parts.back().c_str()); parts.pop_back(); }
        if (f1.eof && (!pe || f2.eof)) break;
        want *= 2;
        continue;
      }
      want = want0;
      f1.drop(u1);
      f2.drop(u2);
      if (whole) break;
    }
    return 0;
  }

  // -H: the four totals LoadRawReads logs behind the reads (KAligner.cpp:12392-12413), over every rank of a -G run
  int report_contaminants() {
    if (!o.contam_tbl) return 0;
    if (pl) CK(k4_pipeline_contam_totals(pl, n_contam));
    if (comm && k4_comm_allreduce_sum_u64(comm, n_contam, 4) != K4_OK) { fprintf(stderr, "k4align: rank %d: all-reduce failed: %s\n", o.rank, k4_comm_last_error(comm)); return 2; }
    if (chatty) {
      fprintf(stderr, "k4align: %llu 5' and %llu 3' contaminant trimmed %s reads\n", (unsigned long long)n_contam[0], (unsigned long long)n_contam[1], pe ? "PE1" : "SE");
      if (pe) fprintf(stderr, "k4align: %llu 5' and %llu 3' contaminant trimmed PE2 reads\n", (unsigned long long)n_contam[2], (unsigned long long)n_contam[3]);
    }
    return 0;
  }

  // ---- statistics (ReportAlignStats) ------------------------------------------------------------------------------------------
  int tally() {
    my_lines = tot.n_lines;
    if (n_loci > 0) {  // the EN line is m_NumSloughedNs, counted while the reads are aligned (KAligner.cpp:3732): a PE mate marked LC since stays in it
      uint64_t prior[20];
      CK(k4_filter_marked_prior(ix, prior));
      tot.nar[K4_NAR_NS] += prior[K4_NAR_NS];
    }
    if (comm) {  // the final aligned-read count/merge: one all-reduce of the tallies (north_star: the only collective on the path)
      uint64_t t[26];
      for (int k = 0; k < 20; k++) t[k] = tot.nar[k];
      t[20] = tot.plus; t[21] = tot.minus; t[22] = tot.n_lines; t[23] = n_under; t[24] = n_over; t[25] = n_units;
      if (k4_comm_allreduce_sum_u64(comm, t, 26) != K4_OK) { fprintf(stderr, "k4align: rank %d: all-reduce failed: %s\n", o.rank, k4_comm_last_error(comm)); return 2; }
      for (int k = 0; k < 20; k++) tot.nar[k] = t[k];
      tot.plus = t[20]; tot.minus = t[21]; tot.n_lines = t[22]; n_under = t[23]; n_over = t[24]; n_units = t[25];
    }
    const uint64_t n_loaded = (uint64_t)(pe ? 2 : 1) * (n_units - n_under - n_over);
    if (chatty) {
      fprintf(stderr, "k4align: From %llu source reads there are %llu accepted alignments, %llu on '+' strand, %llu on '-' strand\n",
              (unsigned long long)n_loaded, (unsigned long long)tot.nar[1], (unsigned long long)tot.plus, (unsigned long long)tot.minus);
      if (n_under || n_over)
        fprintf(stderr, "k4align: %llu under length and %llu over length reads were sloughed\n", (unsigned long long)n_under,
                (unsigned long long)n_over);
      for (int k = 0; k < 20; k++) fprintf(stderr, "k4align:    %llu (%s)\n", (unsigned long long)tot.nar[k], kNarAbbr[k]);
    }
    return 0;
  }

  // ---- the output ----------------------------------------------------------------------------------------------------------------
  // the formatted records come down piece by piece (the previous piece is written meanwhile); a sink that fails has said why
  template <class Sink> int drain_sam(Sink sink) {
    for (;;) {
      const void* ptr = nullptr;
      uint64_t len = 0;
      CK(k4_pipeline_next_sam(pl, &ptr, &len));
      if (len == 0) return 0;
      if (!sink(ptr, len)) return 5;
    }
  }
  // every sequence of the index in turn, and whether the header declares it: all of them, or only the ones with alignments
  template <class Each> void walk_dictionary(bool all, Each each) {
    for (uint32_t c = 1; c <= info.n_entries; c++) {
      k4_entry e;
      k4_get_entry(ix, c, &e);
      each(c, e, all || hit_chrom[c]);
    }
  }
  // A rank of a -G run whose output is BAM: its coordinate-sorted BAM records as they are (refID = sequence number - 1), and beside
  // them the dictionary with this rank's hit flags; the parent merges the ranks' streams into the one BAM file (run_multi_gpu)
  int write_rank_bam() {
    FILE* fp = fopen(o.out.c_str(), "wb");
    if (!fp) { fprintf(stderr, "k4align: unable to create %s\n", o.out.c_str()); return 5; }
    made.push_back(o.out);
    made.push_back(o.out + ".sq");
    uint64_t nbytes = 0;
    int rc = drain_sam([&](const void* ptr, uint64_t len) { nbytes += len; return fwrite(ptr, 1, (size_t)len, fp) == (size_t)len; });
    if (fclose(fp) != 0 && rc == 0) rc = 5;
    if (rc == 5) fprintf(stderr, "k4align: unable to write %s\n", o.out.c_str());
    if (rc != 0) return rc;
    FILE* fd = fopen((o.out + ".sq").c_str(), "wb");
    if (!fd) { fprintf(stderr, "k4align: unable to create %s.sq\n", o.out.c_str()); return 5; }
    fprintf(fd, "%s\n", info.dataset);
    walk_dictionary(false, [&](uint32_t, const k4_entry& e, bool hit) { fprintf(fd, "%s\t%u\t%d\n", e.name, e.seq_len, hit ? 1 : 0); });
    if (fclose(fd) != 0) { fprintf(stderr, "k4align: unable to write %s.sq\n", o.out.c_str()); return 5; }
    ok = true;
    if (chatty) fprintf(stderr, "k4align: rank %d: %llu alignments as BAM records (%llu bytes) for the merge\n", o.rank, (unsigned long long)my_lines, (unsigned long long)nbytes);
    return 0;
  }
  // BAM (+ .bai): dictionary and BGZF blocks here (include/k4_bam.hpp), the records as packed on the device
  int write_bam() {
    auto tw = now();
    std::string hdr = "@HD\tVN:1.4\tSO:coordinate\n";
    std::vector<k4bam::RefSeq> refs;
    walk_dictionary(few_seqs(), [&](uint32_t, const k4_entry& e, bool declared) {
      if (!declared) return;
      hdr += std::string("@SQ\tAS:") + info.dataset + "\tSN:" + e.name + "\tLN:" + std::to_string(e.seq_len) + "\n";
      refs.push_back({e.name, e.seq_len});
    });
    hdr += "@PG\tID:k4align\tVN:1.0\n";
    k4bam::Writer bw;
    if (!bw.open(o.out, hdr, refs, o.bam_level, std::max(o.io_threads, 1))) { fprintf(stderr, "k4align: %s\n", bw.error().c_str()); return 5; }
    made.push_back(o.out);
    made.push_back(o.out + ".bai");
    const int rc = drain_sam([&](const void* ptr, uint64_t len) { return bw.write(ptr, (size_t)len); });  // (deflated and written meanwhile)
    if (rc == 5 || (rc == 0 && !bw.close())) { fprintf(stderr, "k4align: %s\n", bw.error().c_str()); return 5; }
    if (rc != 0) return rc;
    if (!bw.indexed() && chatty) fprintf(stderr, "k4align: a sequence of 512 Mbp or more: no .bai written (the reference writes a CSI index there)\n");
    if (bw.n_records() != my_lines) { fprintf(stderr, "k4align: internal error: %llu BAM records for %llu alignments\n", (unsigned long long)bw.n_records(), (unsigned long long)my_lines); return 5; }
    reset_pipeline();
    ok = true;
    const double s_write_bam = secs(tw, now());
    if (chatty)
      fprintf(stderr, "k4align: %llu alignments reported to %s (%llu bytes) + .bai; index %.2fs, reads %.2fs, device side behind the reads %.2fs, "
                      "global stages + sort + records %.2fs, deflate + write %.2fs\n", (unsigned long long)bw.n_records(), o.out.c_str(),
              (unsigned long long)bw.compressed_bytes() + 28, index_secs(), s_read, s_parse, s_align, s_write_bam);
    return 0;
  }
  // the SAM body out of the pipeline; a seekable file takes every piece by concurrent writes at its place
  int sam_body_from_pipeline(FILE* fp) {
    fflush(fp);
    const int fd = fileno(fp);
    const bool seekable = lseek(fd, 0, SEEK_CUR) != (off_t)-1;  // (-o /dev/stdout, a pipe: written in order by one thread)
    uint64_t fpos = seekable ? (uint64_t)ftello(fp) : 0;
    if (seekable && ftruncate(fd, (off_t)(fpos + pl_sam_bytes)) != 0) { /* (the size is only a hint for the file system) */ }
    const int rc = drain_sam([&](const void* ptr, uint64_t len) {
      const bool done = seekable ? io_parallel<true>(fd, (uint8_t*)ptr, fpos, len, o.io_threads)
                                 : fwrite(ptr, 1, (size_t)len, fp) == (size_t)len;
      if (!done) fprintf(stderr, "k4align: write to %s failed\n", o.out.c_str());
      fpos += len;
      return done;
    });
    if (rc != 0) return rc;
    if (seekable) fseeko(fp, (off_t)fpos, SEEK_SET);
    auto tc0 = now();
    reset_pipeline();
    if (getenv("K4_TRACE")) fprintf(stderr, "[k4 trace] pipeline closed in %.2fs\n", secs(tc0, now()));
    return 0;
  }
  // -b: every part is coordinate sorted; merge by (chromosome, position), equal keys in batch order = load order
  int merge_parts(FILE* fp, const std::map<std::string, long>& order) {
    struct Src { FILE* f; std::string line; long chrom, pos; };
    std::vector<Src> src(parts.size());
    auto next = [&](Src& x) -> bool {
      x.line.clear();
      char buf[1 << 16];
      while (fgets(buf, sizeof(buf), x.f)) {
        x.line += buf;
        if (!x.line.empty() && x.line.back() == '\n') break;
      }
      if (x.line.empty()) return false;
      size_t a = x.line.find('\t'), b = a == std::string::npos ? a : x.line.find('\t', a + 1);
      size_t c = b == std::string::npos ? b : x.line.find('\t', b + 1);
      if (c == std::string::npos) return false;
      auto it = order.find(x.line.substr(b + 1, c - b - 1));
      x.chrom = it == order.end() ? LONG_MAX : it->second;
      x.pos = atol(x.line.c_str() + c + 1);
      return true;
    };
    typedef std::pair<std::pair<long, long>, int> Item;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> pq;
    for (size_t i = 0; i < parts.size(); i++) {
      src[i].f = fopen(parts[i].c_str(), "rb");
      if (!src[i].f) { fprintf(stderr, "k4align: unable to reopen %s\n", parts[i].c_str()); return 5; }
      if (next(src[i])) pq.push({{src[i].chrom, src[i].pos}, (int)i});
    }
    while (!pq.empty()) {
      const int i = pq.top().second;
      pq.pop();
      fputs(src[i].line.c_str(), fp);
      if (next(src[i])) pq.push({{src[i].chrom, src[i].pos}, i});
    }
    for (size_t i = 0; i < parts.size(); i++) { fclose(src[i].f); remove(parts[i].c_str()); }
    return 0;
  }
  // SAM: header here; the body as formatted on the device -- from the pipeline, the kept block of the single batch, or the parts
  int write_sam() {
    auto tw = now();
    FILE* fp = fopen(o.out.c_str(), "wb");
    if (!fp) { fprintf(stderr, "k4align: unable to create %s\n", o.out.c_str()); return 5; }
    made.push_back(o.out);
    static char iobuf[1 << 22];
    setvbuf(fp, iobuf, _IOFBF, sizeof(iobuf));
    fprintf(fp, "@HD\tVN:1.4\tSO:coordinate\n");
    // a shard (-S, -G) declares every sequence and leaves the rule to the merge, which sees every shard's records
    std::map<std::string, long> order;
    walk_dictionary(few_seqs() || o.n_shards > 1 || multi, [&](uint32_t c, const k4_entry& e, bool declared) {
      order.emplace(e.name, (long)c);
      if (declared) fprintf(fp, "@SQ\tAS:%s\tSN:%s\tLN:%u\n", info.dataset, e.name, e.seq_len);
    });
    fprintf(fp, "@PG\tID:k4align\tVN:1.0\n");
    int rc = 0;
    if (pl) rc = sam_body_from_pipeline(fp);
    else if (keep_sam) CK(download(ix, keep_sam.get(), keep_bytes, fp));
    else if (!parts.empty()) rc = merge_parts(fp, order);
    if (rc != 0) return rc;
    fflush(fp);
    const bool wfail = ferror(fp) != 0;
    if (fclose(fp) != 0 || wfail) { fprintf(stderr, "k4align: write to %s failed\n", o.out.c_str()); return 5; }
    s_write += secs(tw, now());
    fprintf(stderr, "k4align: %s%llu alignments written to %s (%zu batch%s); index %.2fs, read files %.2fs, upload+parse %.2fs, align+format %.2fs, write %.2fs\n",
            multi ? ("rank " + std::to_string(o.rank) + ": ").c_str() : "", (unsigned long long)my_lines, o.out.c_str(),
            parts.empty() ? (size_t)1 : parts.size(), parts.size() > 1 ? "es" : "", index_secs(), s_read, s_parse, s_align, s_write);
    ok = true;
    if (comm) {  // (closed behind the index: RunHeld)
      k4_comm_barrier(comm);
      met_peers = true;
    }
    return 0;
  }
};

// CKAligner::Align's steps (KAligner.cpp:391-800) in its order: index, parameters, reads + alignment, the stages over all reads,
// the reports, the statistics, the alignments
static int run_rank(Opts& o, const bool pe, const int max_ml) {
  Run r(o, pe, max_ml);
  int rc;
#define STEP(call) if ((rc = r.call) != 0) return rc
  STEP(open_index());
  STEP(load_constraints());
  STEP(derive_params());
  if (r.pipelined) {
    STEP(open_pipeline());
    STEP(feed_pipeline());
    STEP(report_contaminants());
    auto tg = now();
    const k4_pipeline_view& v = r.v;
    STEP(global_stages(v.n_units, v.max_read_len, v.d_rr, v.d_hits, v.d_seg2, v.d_pe, v.d_reads, v.d_offs, v.d_lens));
    STEP(write_unaligned());                                 // -j / -J: before the alignments are reported
    if (o.fmode == 3) return r.write_pba();                  // -M3: that is the report
    if (o.min_snp_reads > 0) STEP(write_snps());             // -p, -S, -K, -7
    if (!o.stats_file.empty()) STEP(write_align_stats());    // -O
    if (o.pe_insert_dist) STEP(write_pe_insert_dist());      // -3
    if (!o.site_file.empty()) STEP(write_site_prefs());      // -8
    STEP(format_records());
    r.s_align = secs(tg, now());
  } else {
    STEP(stream_batches());
    STEP(report_contaminants());
  }
  STEP(tally());
#undef STEP
  return o.rank_bam ? r.write_rank_bam() : r.bam_out ? r.write_bam() : r.write_sam();
}

// k4align -G g0,g1,...: the parent forks one rank per GPU BEFORE anything touches HIP and only waits and merges; the ranks
// form an RCCL communicator (the id travels through a shared anonymous mapping), rank 0 reads the .sfx once and every rank
// receives sequence + suffix array over xGMI (k4_comm_open_index), each aligns its contiguous slice of the reads, the NAR
// tallies are summed with one all-reduce, and the parent merges the ranks' coordinate-sorted shards.
// The ranks' record streams + dictionaries -> the one BAM file: header by kalign's @SQ rule over the union of the ranks' hit
// flags (m_MaxRptSAMSeqsThres, KAligner.cpp:5785-5821), records merged by (refID, pos) with equal keys in rank order -- the order
// the reads were loaded in -- renumbered when not every sequence is declared, deflated and indexed by k4bam::Writer.
static int merge_rank_bams(const std::vector<std::string>& shards, const std::string& out, const Opts& o, unsigned long long* n_out) {
  std::string dataset;
  std::vector<k4bam::RefSeq> all;
  std::vector<char> hit;
  for (size_t r = 0; r < shards.size(); r++) {
    FILE* fd = fopen((shards[r] + ".sq").c_str(), "rb");
    if (!fd) { fprintf(stderr, "k4align: unable to open %s.sq\n", shards[r].c_str()); return 5; }
    char line[512];
    size_t c = 0;
    bool first = true, ok = true;
    while (ok && fgets(line, sizeof(line), fd)) {
      size_t L = strlen(line);
      if (L && line[L - 1] == '\n') line[--L] = 0;
      if (first) { if (r == 0) dataset = line; first = false; continue; }
      char* t1 = strchr(line, '\t');
      char* t2 = t1 ? strchr(t1 + 1, '\t') : nullptr;
      if (!t2) { ok = false; break; }
      *t1 = 0; *t2 = 0;
      if (r == 0) { all.push_back({line, (uint32_t)strtoul(t1 + 1, nullptr, 10)}); hit.push_back(0); }
      else if (c >= all.size() || all[c].name != line) { ok = false; break; }
      if (t2[1] == '1') hit[c] = 1;
      c++;
    }
    fclose(fd);
    if (!ok || c != all.size()) { fprintf(stderr, "k4align: %s.sq does not match the other ranks' dictionaries\n", shards[r].c_str()); return 5; }
  }
  const bool all_sq = all.size() <= (size_t)o.rpt_sq_thres;
  std::string hdr = "@HD\tVN:1.4\tSO:coordinate\n";
  std::vector<k4bam::RefSeq> refs;
  std::vector<int32_t> ref_map(all.size(), -1);
  for (size_t c = 0; c < all.size(); c++) {
    if (!(all_sq || hit[c])) continue;
    ref_map[c] = (int32_t)refs.size();
    hdr += "@SQ\tAS:" + dataset + "\tSN:" + all[c].name + "\tLN:" + std::to_string(all[c].len) + "\n";
    refs.push_back(all[c]);
  }
  hdr += "@PG\tID:k4align\tVN:1.0\n";
  k4bam::Writer bw;
  if (!bw.open(out, hdr, refs, o.bam_level, std::max(o.io_threads, 1) * (int)shards.size())) { fprintf(stderr, "k4align: %s\n", bw.error().c_str()); return 5; }
  std::string why;
  const int rc = k4merge::merge_bam_records(shards, all_sq ? nullptr : &ref_map, [&](const void* p, size_t n) { return bw.write(p, n); }, n_out, &why);
  if (rc) { fprintf(stderr, "k4align: %s\n", why.empty() ? bw.error().c_str() : why.c_str()); return rc; }
  if (!bw.close()) { fprintf(stderr, "k4align: %s\n", bw.error().c_str()); return 5; }
  if (bw.n_records() != *n_out) { fprintf(stderr, "k4align: internal error: %llu BAM records written, %llu merged\n", (unsigned long long)bw.n_records(), *n_out); return 5; }
  return 0;
}

static int run_multi_gpu(Opts& o, bool pe, int max_ml) {
  const int N = (int)o.gpus.size();
  if (N > K4_MAX_RANKS) { fprintf(stderr, "k4align: at most %d GPUs\n", K4_MAX_RANKS); return 1; }
  if (o.batch_mb > 0 || o.n_shards > 1 || o.legacy) { fprintf(stderr, "k4align: -G cannot be combined with -b, -S or -Z\n"); return 1; }
  if (o.ml_mode == 2 || o.ml_mode == 3 || o.ml_mode == 4 || o.micro_indel || o.splice_junct) {
    fprintf(stderr, "k4align: -r2 / -r3 / -r4 / -a / -A look at all reads of the run; they cannot be combined with -G\n");
    return 1;
  }
  if (o.in1.size() > K4_MAX_FILES || o.in2.size() > K4_MAX_FILES) { fprintf(stderr, "k4align: -G takes at most %d reads files per end\n", K4_MAX_FILES); return 1; }
  MultiShared* sh = (MultiShared*)mmap(nullptr, sizeof(MultiShared), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
  if (sh == MAP_FAILED) { fprintf(stderr, "k4align: unable to map shared memory\n"); return 2; }
  memset((void*)sh, 0, sizeof(*sh));
  const std::string final_out = o.out;
  const bool bam_final = final_out.size() >= 4 && strcasecmp(final_out.c_str() + final_out.size() - 4, ".bam") == 0;
  auto t0 = std::chrono::steady_clock::now();
  // fault injection for the tests of this function (K4ALIGN_FAULT=<rank>:<stage>): the named rank leaves with exit code 3 at
  // "start" (before the communicator exists) / "index" (after the broadcast of the index); with K4ALIGN_FAULT_PEERS=block the
  // other ranks then behave like ranks blocked inside a collective -- they wait for ever -- so that a machine without GPUs can
  // show that the parent ends a run one of whose ranks died
  std::vector<pid_t> kids;
  bool fork_failed = false;
  for (int r = 0; r < N; r++) {
    const pid_t pid = fork();
    if (pid < 0) { fprintf(stderr, "k4align: fork failed\n"); sh->failed = 1; fork_failed = true; break; }
    if (pid == 0) {
      o.rank = r; o.n_ranks = N; o.gpu = o.gpus[(size_t)r]; o.shared = sh;
      o.out = final_out + ".rank" + std::to_string(r);
      o.rank_bam = bam_final;
      const int rc = run_rank(o, pe, max_ml);
      if (rc != 0) sh->failed = 1;
      fflush(nullptr);
      _exit(rc);
    }
    kids.push_back(pid);
  }
  // The ranks meet in collectives: one that dies (or never started) leaves its peers waiting inside RCCL for ever.  So the
  // parent reaps whichever child ends first; at the first failure -- a non-zero exit, a signal, a fork that failed -- the
  // others are killed and reaped, the shards removed, and the run ends with that failure's code within moments.
  int worst = fork_failed ? 2 : 0;
  size_t alive = kids.size();
  auto kill_rest = [&]() {
    for (pid_t k : kids)
      if (k > 0) kill(k, SIGKILL);
  };
  if (fork_failed) kill_rest();
  while (alive) {
    int st = 0;
    const pid_t done = waitpid(-1, &st, 0);
    if (done < 0) { if (errno == EINTR) continue; break; }
    bool ours = false;
    for (pid_t& k : kids)
      if (k == done) { k = -1; ours = true; }
    if (!ours) continue;
    alive--;
    const int rc = WIFEXITED(st) ? WEXITSTATUS(st) : 9;
    if (rc && !worst) {
      worst = rc;
      fprintf(stderr, "k4align: a rank %s (%d): ending the others\n", WIFEXITED(st) ? "failed" : "was killed", WIFEXITED(st) ? rc : WTERMSIG(st));
      kill_rest();
    }
  }
  std::vector<std::string> shards;
  for (int r = 0; r < N; r++) shards.push_back(final_out + ".rank" + std::to_string(r));
  if (worst || sh->failed) {
    for (const std::string& q : shards) { remove(q.c_str()); remove((q + ".sq").c_str()); }
    munmap((void*)sh, sizeof(*sh));
    return worst ? worst : 2;
  }
  auto t1 = std::chrono::steady_clock::now();
  unsigned long long n = 0;
  if (bam_final) {
    const int rc = merge_rank_bams(shards, final_out, o, &n);
    for (const std::string& q : shards) { remove(q.c_str()); remove((q + ".sq").c_str()); }
    munmap((void*)sh, sizeof(*sh));
    if (rc) return rc;
    fprintf(stderr, "k4align: %llu alignments from %d GPUs written to %s (+ .bai); ranks %.2fs, merge + deflate %.2fs\n", n, N, final_out.c_str(),
            std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count());
    return 0;
  }
  const int rc = k4merge::merge_sam(shards, final_out, o.rpt_sq_thres, &n, "k4align", std::max(o.io_threads, 1) * N);  // (the ranks' reader threads are idle now)
  for (const std::string& q : shards) remove(q.c_str());
  if (rc) return rc;
  fprintf(stderr, "k4align: %llu alignments from %d GPUs written to %s; ranks %.2fs, merge %.2fs\n", n, N, final_out.c_str(),
          std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count());
  munmap((void*)sh, sizeof(*sh));
  return 0;
}

int main(int argc, char** argv) {
  Opts o;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    if (a.size() < 2 || a[0] != '-') { usage(); return 1; }
    auto val = [&]() -> std::string { return a.size() > 2 ? a.substr(2) : (i + 1 < argc ? std::string(argv[++i]) : std::string()); };
    if (a[1] != '-') o.given += a[1];
    switch (a[1]) {
      case '-': {  // kalign's long names, for the options whose letters are taken here: --name value | --name=value
        std::string name = a.substr(2), v;
        const size_t eq = name.find('=');
        if (name == "petranslendist") { o.pe_insert_dist = true; o.given += '3'; break; }  // the long names that are flags
        if (name == "nofiltpriority") { o.no_filt_priority = true; break; }
        if (eq != std::string::npos) { v = name.substr(eq + 1); name.resize(eq); }
        else if (i + 1 < argc) v = argv[++i];
        else { usage(); return 1; }
        if (name == "chromexclude") o.chrom_excl.push_back(v);
        else if (name == "chromeinclude") o.chrom_incl.push_back(v);
        else if (name == "priorityregionfile") o.priority_file = v;
        else if (name == "lociconstraints") { o.loci_file = v; o.given += '5'; }
        else if (name == "pcrprimersubs") { o.primer_subs = atoi(v.c_str()); o.given += '6'; }
        else if (name == "siteprefs") { o.site_file = v; o.given += '8'; }
        else if (name == "siteprefsofs") { o.site_ofs = atoi(v.c_str()); o.given += '9'; }
        else if (name == "snpcentroid") { o.cent_file = v; o.given += '7'; }
        else if (name == "markerlen") { o.marker_len = atoi(v.c_str()); o.given += 'K'; }
        else if (name == "markerpolythres") { o.marker_poly_thres = atof(v.c_str()); o.marker_thres_given = true; o.given += 'K'; }
        else if (name == "contaminants") { o.contam_file = v; o.given += 'H'; }
        else if (name == "experimentid") { o.experiment_id = clean_id(v); o.given += 'w'; }
        else if (name == "readsetid") { o.readset_id = clean_id(v); o.given += 'W'; }
        else { usage(); return 1; }
        break;
      }
      case '3': o.pe_insert_dist = true; break;
      case '5': o.loci_file = val(); break;
      case '6': o.primer_subs = atoi(val().c_str()); break;
      case 'i': o.in1.push_back(val()); break;
      case 'u': o.in2.push_back(val()); break;
      case 'I': o.sfx = val(); break;
      case 'o': o.out = val(); break;
      case 's': o.max_subs = atoi(val().c_str()); break;
      case 'e': o.min_edit = atoi(val().c_str()); break;
      case 'm': o.pmode = atoi(val().c_str()); break;
      case 'n': o.max_ns = atoi(val().c_str()); break;
      case 'U': o.pe_mode = atoi(val().c_str()); break;
      case 'd': o.pair_min = atoi(val().c_str()); break;
      case 'D': o.pair_max = atoi(val().c_str()); break;
      case 'E': o.pair_strand = 1; break;
      case 'l': o.min_len = atoi(val().c_str()); break;
      case 'L': o.max_len = atoi(val().c_str()); break;
      case 'r': o.ml_mode = atoi(val().c_str()); break;
      case 'R': o.max_multi = atoi(val().c_str()); break;
      case 'c': o.min_chimeric = atoi(val().c_str()); break;
      case 'a': o.micro_indel = atoi(val().c_str()); break;
      case 'A': o.splice_junct = atoi(val().c_str()); break;
      case 'x': o.min_flank_exacts = atoi(val().c_str()); break;
      case 'k': o.pcr_win = atoi(val().c_str()); o.pcr_given = true; break;
      case 'O': o.stats_file = val(); break;
      case '8': o.site_file = val(); break;
      case '9': o.site_ofs = atoi(val().c_str()); break;
      case 'p': o.min_snp_reads = atoi(val().c_str()); break;
      case 'P': o.qvalue = atof(val().c_str()); break;
      case '1': o.snp_nonref_pcnt = atof(val().c_str()); break;
      case '7': o.cent_file = val(); break;
      case 'K': o.marker_len = atoi(val().c_str()); break;
      case 'V': o.no_filt_priority = true; break;
      case 'X': o.clamp = true; break;
      case 'N': o.best = true; break;
      case 'S': {  // "i/N": this process's slice of the reads; anything else: kalign's -S, the SNP file
        std::string v = val();
        int sa = 0, sb = 0;
        char tail = 0;
        if (sscanf(v.c_str(), "%d/%d%c", &sa, &sb, &tail) == 2) { o.shard = sa; o.n_shards = sb; }
        else if (v.empty()) { usage(); return 1; }
        else o.snp_file = v;
        break;
      }
      case 'g': o.q_method = atoi(val().c_str()); break;  // kalign's -g: FASTQ quality scoring (0 Sanger, 1 Illumina 1.3+, 2 Solexa, 3 ignore)
      case '@': o.gpu = atoi(val().c_str()); break;
      case 'G': { std::string v = val(); for (size_t q = 0; q < v.size();) { size_t e = v.find(',', q); if (e == std::string::npos) e = v.size(); o.gpus.push_back(atoi(v.substr(q, e - q).c_str())); q = e + 1; } break; }
      case 'b': o.batch_mb = atof(val().c_str()); break;
      case 'B': o.chunk_mb = std::max(1, atoi(val().c_str())); break;
      case 't': o.io_threads = std::max(1, atoi(val().c_str())); break;
      case 'M': o.fmode = atoi(val().c_str()); break;
      case 'Q': o.align_strand = atoi(val().c_str()); break;
      case '4': o.rpt_sq_thres = std::max(1, atoi(val().c_str())); break;
      case 'j': o.none_file = val(); break;
      case 'J': o.multi_file = val(); break;
      case '#': o.sample_nth = std::min(10000, std::max(1, atoi(val().c_str()))); break;
      case 'H': o.contam_file = val(); break;
      case 'y': o.trim5 = atoi(val().c_str()); break;
      case 'Y': o.trim3 = atoi(val().c_str()); break;
      case 'Z': o.legacy = true; break;
      case 'z': o.bam_level = std::min(9, std::max(0, atoi(val().c_str()))); break;
      case 'W': o.print_slices = atoi(val().c_str()); break;
      case 'T': case 'F': (void)val(); break;  // accepted and ignored (threads, log file)
      default: usage(); return 1;
    }
  }
  if (o.print_slices > 0 && !o.in1.empty()) {  // the slice table of a -G run (host only): per end and file, where each rank starts
    if (o.print_slices > K4_MAX_RANKS || o.in1.size() > K4_MAX_FILES || o.in2.size() > K4_MAX_FILES) return 1;
    std::vector<std::vector<uint64_t>> tab[2];
    uint64_t R = 0, R2 = 0;
    std::vector<uint64_t> counts;
    std::string why;
    auto offs = std::unique_ptr<uint64_t[][K4_MAX_RANKS + 1]>(new uint64_t[K4_MAX_FILES][K4_MAX_RANKS + 1]);
    for (int e = 0; e < (o.in2.empty() ? 1 : 2); e++) {
      const std::vector<std::string>& fl = e ? o.in2 : o.in1;
      if (e && o.in2.size() != o.in1.size()) { fprintf(stderr, "k4align: as many -u files as -i files are needed\n"); return 3; }
      if (!slice_files(fl, o.print_slices, counts, e == 1, offs.get(), e ? &R2 : &R, o.io_threads, &why)) { fprintf(stderr, "k4align: %s\n", why.c_str()); return e ? 3 : 2; }
      if (e == 0) printf("records %llu\n", (unsigned long long)R);
      for (size_t f = 0; f < fl.size(); f++) {
        if (fl.size() == 1) printf("end %d", e); else printf("end %d file %d", e, (int)f);
        for (int r = 0; r <= o.print_slices; r++) printf(" %llu", (unsigned long long)offs[f][r]);
        printf("\n");
      }
    }
    return 0;
  }
  if (o.in1.empty() || o.sfx.empty() || o.out.empty()) { usage(); return 1; }
  const bool pe = !o.in2.empty();
  // --priorityregionfile (kalign -B): the priority pass needs AlignReads' own hit limit, which -X clamps and -N does not have; genpba
  // has no such option
  if (!o.priority_file.empty()) {
    if (o.ml_mode == 5 && (o.clamp || o.best)) { fprintf(stderr, "k4align: priority regions '--priorityregionfile' with -r5 -X / -N are not built\n"); return 3; }
    if (o.fmode == 3) { fprintf(stderr, "k4align: priority regions '--priorityregionfile' with packed base alleles '-M3' are not built\n"); return 3; }
    FILE* t = fopen(o.priority_file.c_str(), "rb");
    if (!t) { fprintf(stderr, "k4align: Unable to open high priority regions BED file '%s'\n", o.priority_file.c_str()); return 2; }
    fclose(t);
  }
  // -M3: `ngskit4b genpba` (kalignerPBA, KAlignerCL.cpp:1540-2290).  Its argument table (:1556-1628) is kalign's without the
  // second-segment phases, the side files and SNP calling; -w / -W are required there (arg_str1, cleaned :1697-1729)
  if (o.fmode == 3) {
    for (const char c : std::string("aAOjJ8953pP1N7K"))
      if (o.given.find(c) != std::string::npos) { fprintf(stderr, "k4align: genpba '-M3' has no option '-%c'\n", c); return 1; }
    if (!o.snp_file.empty()) { fprintf(stderr, "k4align: genpba '-M3' calls no SNPs: no SNP file '-S%s'\n", o.snp_file.c_str()); return 1; }
    if (o.given.find('w') == std::string::npos || o.given.find('W') == std::string::npos) {
      fprintf(stderr, "k4align: packed base alleles '-M3' need --experimentid <id> and --readsetid <id>\n");
      return 1;
    }
    if (o.experiment_id.empty()) { fprintf(stderr, "k4align: No experiment identifier specified\n"); return 1; }
    if (o.readset_id.empty()) { fprintf(stderr, "k4align: No readset identifier specified\n"); return 1; }
    const bool bam_name = o.out.size() >= 4 && strcasecmp(o.out.c_str() + o.out.size() - 4, ".bam") == 0;
    if (o.batch_mb > 0 || o.n_shards > 1 || !o.gpus.empty() || o.legacy || o.ml_mode == 5 || bam_name) {
      fprintf(stderr, "k4align: packed base alleles '-M3' pile up the whole run's alignments: with -b, -S i/N, -G, -Z, -r5 or a .bam output name they are not built\n");
      return 3;
    }
  } else if (o.given.find('w') != std::string::npos || o.given.find('W') != std::string::npos) {
    fprintf(stderr, "k4align: --experimentid / --readsetid belong to the packed base alleles output '-M3'\n");
    return 1;
  }
  // multi-loci modes (KAlignerCL.cpp:686-707): 0 slough, 1 statistics only, 5 report every locus up to -R; the modes that
  // pick or cluster one locus (2 random, 3/4 AssignMultiMatches) are not part of this path
  if (o.ml_mode < 0 || o.ml_mode > 5) { fprintf(stderr, "k4align: -r%d is not supported (0..5 are)\n", o.ml_mode); return 1; }
  if (o.ml_mode != 0 && pe) { fprintf(stderr, "k4align: multiloci processing '-r%d' not supported in paired end processing\n", o.ml_mode); return 1; }
  if (o.n_shards < 1 || o.shard < 0 || o.shard >= o.n_shards) { fprintf(stderr, "k4align: -S i/N needs 0 <= i < N\n"); return 1; }
  if ((o.clamp || o.best) && o.ml_mode != 5) { fprintf(stderr, "k4align: -X / -N are supported together with -r5 only\n"); return 1; }
  int max_ml = 1;
  if (o.ml_mode != 0) {
    max_ml = o.max_multi ? o.max_multi : 5;  // cDfltMaxMultiHits
    const int lim = o.ml_mode == 5 ? 100000 : 500;  // cMaxAllHits / cMaxMultiHits
    if (max_ml < 2 || max_ml > lim) { fprintf(stderr, "k4align: -R%d outside of range 2..%d\n", max_ml, lim); return 1; }
  }
  // the optional AlignReads phases and the stages they bring with them: the same argument rules as kalign (KAlignerCL.cpp:545-569,
  // 667-761,823-830)
  o.min_chimeric = abs(o.min_chimeric);
  if (o.min_chimeric != 0 && (o.min_chimeric < 15 || o.min_chimeric > 99)) { fprintf(stderr, "k4align: minimum chimeric length percentage '-c%d' specified outside of range 15..99\n", o.min_chimeric); return 1; }
  if (o.micro_indel < 0 || o.micro_indel > 20) { fprintf(stderr, "k4align: microInDel length maximum '-a%d' specified outside of range 0..20\n", o.micro_indel); return 1; }
  if (o.splice_junct != 0 && (o.splice_junct < 25 || o.splice_junct > 100000)) { fprintf(stderr, "k4align: RNAseq maximum splice junction separation '-A%d' must be either 0 or in the range 25..100000\n", o.splice_junct); return 1; }
  if (o.pcr_given && (o.pcr_win < 0 || o.pcr_win > 250)) {
    fprintf(stderr, "k4align: PCR differential amplification artefacts window length '-k%d' specified outside of range 0..250\n", o.pcr_win);
    return 1;
  }
  // ReducePCRduplicates runs for SE only (KAligner.cpp:628); with -u the option is accepted and does nothing
  if (o.pcr_win >= 0 && !pe) {
    if (o.batch_mb > 0 || o.n_shards > 1 || !o.gpus.empty()) {
      fprintf(stderr, "k4align: -k reduces PCR duplicates over all reads of the run; it cannot be combined with -b, -S or -G\n");
      return 1;
    }
    if (o.ml_mode == 5) { fprintf(stderr, "k4align: PCR artefact reduction '-k' with every multiloci alignment reported '-r5' is not built\n"); return 3; }
  }
  // -6 (KAlignerCL.cpp:803-815; genpba :1975-1987).  The stage looks at one read at a time: it runs with -b, -S i/N and -G as well
  if (o.primer_subs < 0 || o.primer_subs > 5) {
    fprintf(stderr, "k4align: PCR primer correction subs '-6%d' specified outside of range 0..5\n", o.primer_subs);
    return 1;
  }
  if (o.primer_subs != 0 && o.min_chimeric != 0) {
    fprintf(stderr, "k4align: PCR primer correction subs not allowed when also specifying chimeric trimming\n");
    return 1;
  }
  if (o.primer_subs > 0 && o.ml_mode == 5) {  // (there every reported locus is a read of its own to the reference)
    fprintf(stderr, "k4align: PCR primer correction '-6' with every multiloci alignment reported '-r5' is not built\n");
    return 3;
  }
  // -3 is honoured in paired end processing alone and needs -O, whose name its file takes (KAlignerCL.cpp:571-598)
  if (!pe) o.pe_insert_dist = false;
  if (o.pe_insert_dist && o.stats_file.empty()) {
    fprintf(stderr, "k4align: PE insert length distributions requested but no output statistics file '-O<file>' specified\n");
    return 1;
  }
  // the statistics count over all reads of the run in one place (summing per-rank counters is not built)
  if (!o.stats_file.empty()) {
    if (o.batch_mb > 0 || o.n_shards > 1 || !o.gpus.empty() || o.legacy) {
      fprintf(stderr, "k4align: -O counts over all reads of the run; it cannot be combined with -b, -S, -G or -Z\n");
      return 1;
    }
    if (o.ml_mode == 5) { fprintf(stderr, "k4align: alignment statistics '-O' with every multiloci alignment reported '-r5' are not built\n"); return 3; }
  }
  // the site preferences are counted along one walk over all reads of the run (merging the counts of batches or ranks in walk order is not built)
  if (abs(o.site_ofs) > 100) {  // cMaxSitePrefOfs, KAlignerCL.cpp:1054-1058
    fprintf(stderr, "k4align: offset read start sites '-9%d' when processing site octamer preferencing must be in range -100..100\n", o.site_ofs);
    return 1;
  }
  if (!o.site_file.empty() && (o.ml_mode == 5 || o.batch_mb > 0 || o.n_shards > 1 || !o.gpus.empty() || o.legacy)) {
    fprintf(stderr, "k4align: start site octamer preferences '-8' with -r5, -b, -S i/N, -G or -Z are not built\n");
    return 3;
  }
  // the loci constraints and the chromosome filters look at one read (pair) at a time: they run with -b, -S i/N and -G as well
  if (!o.chrom_excl.empty() || !o.chrom_incl.empty()) {
    if (o.chrom_excl.size() > 20 || o.chrom_incl.size() > 20) { fprintf(stderr, "k4align: at most 20 --chromexclude and 20 --chromeinclude expressions\n"); return 1; }  // cMaxExcludeChroms / cMaxIncludeChroms
    for (int which = 0; which < 2; which++)  // a bad expression is a parameter error (CUtility::CompileREs, libkit4b/Utility.cpp:78-140)
      for (const std::string& q : which ? o.chrom_excl : o.chrom_incl) {
        try { std::regex re(q.substr(0, 100)); }
        catch (const std::regex_error& err) {
          fprintf(stderr, "k4align: Unable to compile %s regular expression '%s' - '%s'\n", which ? "exclusion" : "inclusion", q.c_str(), err.what());
          return 1;
        }
      }
    if (pe) { fprintf(stderr, "k4align: --chromexclude / --chromeinclude in paired end processing '-u' (the filter inside ProcessPairedEnds) is not built\n"); return 3; }
    if (o.ml_mode == 5) { fprintf(stderr, "k4align: --chromexclude / --chromeinclude with every multiloci alignment reported '-r5' is not built\n"); return 3; }
  }
  if (!o.loci_file.empty()) {
    if (o.ml_mode == 5) { fprintf(stderr, "k4align: loci base constraints '-5' with every multiloci alignment reported '-r5' are not built\n"); return 3; }
    FILE* t = fopen(o.loci_file.c_str(), "rb");
    if (!t) { fprintf(stderr, "k4align: Unable to open '%s' for processing\n", o.loci_file.c_str()); return 2; }
    fclose(t);
  }
  if (o.q_method < 0 || o.q_method > 3) { fprintf(stderr, "k4align: fastq quality '-g%d' specified outside of range 0..3\n", o.q_method); return 1; }
  if (o.min_flank_exacts < 0 || o.min_flank_exacts > 7) { fprintf(stderr, "k4align: max flank trimming '-x%d' specified outside of range 0..7\n", o.min_flank_exacts); return 1; }
  if (pe && (o.micro_indel || o.splice_junct)) { fprintf(stderr, "k4align: microInDel '-a' / splice junction '-A' processing not supported in paired end processing\n"); return 1; }
  if (o.ml_mode == 5 && (o.micro_indel || o.splice_junct)) { fprintf(stderr, "k4align: microInDels / splice junctions not supported when reporting multiloci alignments '-r5'\n"); return 1; }
  if (o.min_chimeric && (o.best || o.ml_mode == 3 || o.ml_mode == 4)) { fprintf(stderr, "k4align: chimeric read processing cannot be combined with -N / -r3 / -r4\n"); return 1; }
  // output format (KAlignerCL.cpp:217,514-519): -M0 the accepted alignments, -M1 every loaded read, -M3 genpba's packed base
  // alleles (checked above); -M2 (BED) is not built
  if (o.fmode < 0 || o.fmode > 3) { fprintf(stderr, "k4align: output format mode '-M%d' specified outside of range 0..3\n", o.fmode); return 1; }
  if (o.fmode == 2) { fprintf(stderr, "k4align: output format -M2 (BED) is not built\n"); return 3; }
  if (o.fmode == 1) {
    if (o.batch_mb > 0 || o.n_shards > 1 || o.legacy || o.ml_mode == 5) {
      fprintf(stderr, "k4align: -M1 is written by the pipelined modes (not with -b, -S i/N, -Z, -r5)\n");
      return 3;
    }
    if (o.min_snp_reads > 0 || !o.snp_file.empty()) { fprintf(stderr, "k4align: SNP calling is not available in '-M1' output mode\n"); return 1; }  // KAlignerCL.cpp:935
  }
  // SNP calling (KAlignerCL.cpp:877-945): -S alone means -p20; -p alone writes <out>.snp; -P defaults to 0.05
  if (!o.snp_file.empty() && o.min_snp_reads == 0) o.min_snp_reads = 20;
  if (o.min_snp_reads != 0 && (o.min_snp_reads < 1 || o.min_snp_reads > 100)) { fprintf(stderr, "k4align: minimum read coverage at any loci '-p%d' must be in range 1..100\n", o.min_snp_reads); return 1; }
  if (o.min_snp_reads > 0) {
    if (o.snp_file.empty()) o.snp_file = o.out + ".snp";
    if (o.qvalue < 0.0 || o.qvalue > 0.40) { fprintf(stderr, "k4align: QValue '-P%1.5f' for controlling SNP FDR (Benjamini-Hochberg) must be in range 0.0 to 0.4\n", o.qvalue); return 1; }
    if (o.qvalue == 0.0) o.qvalue = 0.05;
    if (o.snp_nonref_pcnt < 0.1 || o.snp_nonref_pcnt > 35.0) { fprintf(stderr, "k4align: SNP minimum non-ref '-1%f' must be in range 0.1 to 35.0\n", o.snp_nonref_pcnt); return 1; }
    if (o.ml_mode == 5) { fprintf(stderr, "k4align: SNP processing is not supported when reporting all multiloci alignments '-r5'\n"); return 1; }
    if (o.batch_mb > 0 || o.n_shards > 1 || !o.gpus.empty() || o.legacy) { fprintf(stderr, "k4align: SNP calling runs over the whole run's alignments: not with -b, -S i/N, -G, -Z\n"); return 3; }
  }
  // marker sequences and SNP centroids (KAlignerCL.cpp:949-983; the range test keeps the reference's precedence: only -K0 means none)
  if ((o.marker_len != 0 && o.marker_len < 25) || o.marker_len > 500) { fprintf(stderr, "k4align: Marker length specified with '-K%d' must be in range 25 to 500\n", o.marker_len); return 1; }
  if (o.marker_len) {
    if (!o.marker_thres_given) o.marker_poly_thres = 1.0 / 3.0;  // cDfltMinMarkerSNPProp
    if (o.marker_poly_thres < 0.0 || o.marker_poly_thres > 0.50) {
      fprintf(stderr, "k4align: Max marker sequence base polymorphism specified with '--markerpolythres %1.3f' must be in range 0.0 to 0.5\n", o.marker_poly_thres);
      return 1;
    }
  } else
    o.marker_poly_thres = 0.0;
  // (kalign opens both files without SNP calling and leaves them empty; here that is an error)
  if ((o.marker_len || !o.cent_file.empty()) && o.min_snp_reads == 0) {
    fprintf(stderr, "k4align: marker sequences '-K' and SNP centroids '-7' are written by SNP calling: give '-p<n>' or '-S<file>'\n");
    return 1;
  }
  if (o.splice_junct > 0 && o.min_chimeric == 0 && o.min_flank_exacts == 0) o.min_flank_exacts = o.max_subs;  // "force flank trim", :829-830
  if (o.min_flank_exacts > 7) o.min_flank_exacts = 7;
  if ((!o.none_file.empty() || !o.multi_file.empty()) && (o.batch_mb > 0 || o.n_shards > 1 || !o.gpus.empty() || o.legacy)) {
    fprintf(stderr, "k4align: -j / -J are written by the pipelined single-GPU mode (not with -b, -S i/N, -G, -Z)\n");
    return 3;
  }
  if (o.sample_nth > 1 && (o.in1.size() > 1 || o.batch_mb > 0 || o.n_shards > 1 || !o.gpus.empty() || o.legacy)) {
    fprintf(stderr, "k4align: -#%d samples the reads of ONE input file per end in the pipelined single-GPU mode (not with several -i files, -b, -S i/N, -G, -Z)\n", o.sample_nth);
    return 3;
  }
  if (o.trim5 < 0 || o.trim5 > 50) { fprintf(stderr, "k4align: Trim 5' raw reads '-y%d' specified outside of range 0..50\n", o.trim5); return 1; }
  if (o.trim3 < 0 || o.trim3 > 50) { fprintf(stderr, "k4align: Trim 3' raw reads '-Y%d' specified outside of range 0..50\n", o.trim3); return 1; }
  if (o.align_strand < 0 || o.align_strand > 2) { fprintf(stderr, "k4align: Aligned to strand '-Q%d' specified outside of range 0..2\n", o.align_strand); return 1; }
  // kalign's argument rules for the alignment proper (KAlignerCL.cpp:546-553,645-657,789-821)
  if (o.min_len < 15 || o.min_len > 2000) { fprintf(stderr, "k4align: minimum accepted read length '-l%d' specified outside of range 15..2000\n", o.min_len); return 1; }  // cMinSeqLen..cMaxSeqLen, :776-786
  if (o.max_len < o.min_len || o.max_len > 2000) { fprintf(stderr, "k4align: maximum accepted read length '-L%d' specified outside of range %d..2000\n", o.max_len, o.min_len); return 1; }
  if (o.pmode < 0 || o.pmode > 3) { fprintf(stderr, "k4align: Processing mode '-m%d' specified outside of range 0..3\n", o.pmode); return 1; }
  if (o.min_edit < 1 || o.min_edit > 2) { fprintf(stderr, "k4align: Minimum edit distance '-e%d' specified outside of range 1..2\n", o.min_edit); return 1; }
  if (o.max_subs < 0 || o.max_subs > 15) { fprintf(stderr, "k4align: Max allowed substitutions per 100bp read length '-s%d' specified outside of range 0..15\n", o.max_subs); return 1; }
  if (o.max_ns < 0 || o.max_ns > 5) { fprintf(stderr, "k4align: Allowed number of indeterminate bases in reads '-n%d' specified outside of range 0..5\n", o.max_ns); return 1; }
  if (pe && o.pe_mode == 0) {  // "-u" without "-U": unique alignments only
    o.pe_mode = 2;
    fprintf(stderr, "k4align: PE2 file(s) with '-u<files>' specified, defaulting PE processing mode to unique alignments only '-U2'\n");
  }
  if (!pe) o.pe_mode = 0;
  if (pe) {
    if (o.pe_mode < 1 || o.pe_mode > 4) { fprintf(stderr, "k4align: PE processing mode '-U%d' specified outside of range 0..4\n", o.pe_mode); return 1; }
    if (o.pair_min < 25 || o.pair_min > 100000) { fprintf(stderr, "k4align: paired end apparent min length '-d%d' must be in range 25..100000\n", o.pair_min); return 1; }
    if (o.pair_max < 0) o.pair_max = std::max(1000, o.pair_min);  // max(cDfltPairMaxLen, PairMinLen)
    if (o.pair_max < std::max(1, o.pair_min) || o.pair_max > 100000) { fprintf(stderr, "k4align: paired end apparent max length '-D%d' must be in range %d..100000\n", o.pair_max, std::max(1, o.pair_min)); return 1; }
  } else if (o.pair_max < 0) o.pair_max = 1000;

  // -H: the contaminants are loaded before the index and the reads (KAligner.cpp:284-301); a file that is turned down ends the run here
  if (!o.contam_file.empty()) {
    char why[256];
    const int rc = k4_load_contaminants(nullptr, o.contam_file.c_str(), &o.contam_tbl, &o.n_contam_tbl, why);
    if (rc != K4_OK) {
      fprintf(stderr, "k4align: %s (%d)\n", why, rc);
      if (rc == K4_ERR_UNSUPPORTED) return 3;
      fprintf(stderr, "k4align: Unable to load contaminate sequences file '%s'\n", o.contam_file.c_str());
      return rc == K4_ERR_OPEN_FILE ? 2 : 1;
    }
    fprintf(stderr, "k4align: %d flank contaminant sequences loaded from '%s'\n", (int)o.n_contam_tbl, o.contam_file.c_str());
  }
  if (!o.gpus.empty()) return run_multi_gpu(o, pe, max_ml);
  return run_rank(o, pe, max_ml);
}
