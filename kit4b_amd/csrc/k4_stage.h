// kit4b_amd/csrc/k4_stage.h -- what a device stage needs on the host side: the view of the records it works on, its scratch
// buffers, the rocPRIM calls with their temporary, the list of the reads a predicate accepts, a counter brought down.
// A new stage starts from here: k4s_read_set checks its record arguments and fills the K4ReadSet (k4_device.h) its kernels take by
// value; they ask the view whether a read was accepted and where its hit is, and take a read out of the report with its reject().
//
// The helpers are templates over the buffer type B: K4DevBuf (k4_pool.h), or the pool-backed Buf of k4_io.hip (k4_pool.h says why the
// ingest / emit stages free nothing).  B needs `p`, `hipError_t alloc(size_t)` (which lets go of what it held) and `as<T>()`;
// a helper's temporary is a B as well, so a stage never mixes the two kinds.  All of them return a K4_* code.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>  // (rocprim/iterator/texture_cache_iterator.hpp calls memset without it)
#include <type_traits>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "k4_device.h"
#include "k4_internal.h"
#include "k4_pool.h"

#define K4_TRY(call)                 \
  do {                               \
    int _try = (call);               \
    if (_try != K4_OK) return _try;  \
  } while (0)

// one trivially copyable value (a counter, a small array of them) from the device, waited for
template <typename T>
int k4s_read_back(k4_index* ix, T* host, const void* dev, hipStream_t st) {
  static_assert(std::is_trivially_copyable<T>::value, "k4s_read_back copies bytes");
  K4_HIP(ix, hipMemcpyAsync(host, dev, sizeof(T), hipMemcpyDeviceToHost, st));
  K4_HIP(ix, hipStreamSynchronize(st));
  return K4_OK;
}

// The sequence batch of a host-pointer search call (sequence i: lens[i] bytes at seqs + offs[i]) sent up on the index's stream into
// ix->seq_stage; *max_len (may be null) = the longest.  The buffers grow without a wait: only that stream uses them, and every call
// that does ends with it waited for.
inline int k4s_stage_seqs(k4_index* ix, int64_t n, const uint8_t* seqs, const uint64_t* offs, const uint32_t* lens, uint32_t* max_len) {
  uint64_t bytes = 0;
  uint32_t longest = 0;
  for (int64_t i = 0; i < n; i++) {
    bytes = bytes > offs[i] + lens[i] ? bytes : offs[i] + lens[i];
    longest = longest > lens[i] ? longest : lens[i];
  }
  if (max_len) *max_len = longest;
  K4SeqStage& s = ix->seq_stage;
  K4_HIP(ix, s.seqs.reserve((size_t)bytes + 16));
  K4_HIP(ix, s.offs.reserve((size_t)(n + 1) * 8));
  K4_HIP(ix, s.lens.reserve((size_t)(n + 1) * 4));
  if (n > 0) {
    K4_HIP(ix, hipMemcpyAsync(s.seqs.p, seqs, (size_t)bytes, hipMemcpyHostToDevice, ix->stream));
    K4_HIP(ix, hipMemcpyAsync(s.offs.p, offs, (size_t)n * 8, hipMemcpyHostToDevice, ix->stream));
    K4_HIP(ix, hipMemcpyAsync(s.lens.p, lens, (size_t)n * 4, hipMemcpyHostToDevice, ix->stream));
  }
  return K4_OK;
}

// The frame of a host-pointer search call.  The opener: the index's device made current, *st = the index's stream, waited for --
// the staged batch, the out buffer and the tables the call is about to replace may still be read by the batch before.  Between
// the two the entry point stages (k4s_stage_seqs), reserves its out buffer, runs what its *_dev form runs and queues the copies
// down.  The closer: the stream waited for and the timer's open section, if there is one, read.  A *_dev form ends with the closer
// on its caller's stream.
inline int k4s_call_open(k4_index* ix, hipStream_t* st) {
  K4_HIP(ix, hipSetDevice(ix->device));
  *st = ix->stream;
  K4_HIP(ix, hipStreamSynchronize(*st));
  return K4_OK;
}
inline int k4s_call_close(k4_index* ix, hipStream_t st, K4Timer& timer) {
  K4_HIP(ix, hipStreamSynchronize(st));
  K4_HIP(ix, timer.read());
  return K4_OK;
}

// kernel<EL> for the index's 4- or 5-byte suffix elements
#define K4S_LAUNCH_EL(ix, kernel, grid, block, st, ...)                                                   \
  do {                                                                                                    \
    if ((ix)->d.el == 4) hipLaunchKernelGGL(kernel<4>, dim3(grid), dim3(block), 0, st, __VA_ARGS__);      \
    else hipLaunchKernelGGL(kernel<5>, dim3(grid), dim3(block), 0, st, __VA_ARGS__);                      \
  } while (0)

// What a stage needs of its record arguments besides the records themselves (SE: d_rr, PE: d_pe): the SE hit slots, the read
// bytes with their offsets and lengths, the SE second segments.  K4RS_UNITS: the count is in SE reads or PE pairs, not in reads.
enum : unsigned { K4RS_HITS = 1u, K4RS_READS = 2u, K4RS_SEG2 = 4u, K4RS_UNITS = 8u };

// The record arguments of a C ABI entry point, checked and made into the view.  An entry point that takes one d_rr_or_pe hands it
// in as d_rr and as d_pe.  What the stage does not need may be null and is carried along as it came; the side of the other record
// form is left out of the view.  An empty call (n <= 0) is not refused.
inline int k4s_read_set(k4_index* ix, int pe, int64_t n, const void* d_rr, const void* d_hits, int32_t max_ml, const void* d_pe,
                        const void* d_seg2, const void* d_reads, const void* d_offs, const void* d_lens, unsigned need, K4ReadSet* rs) {
  const bool records = pe ? d_pe != nullptr : (d_rr && (!(need & K4RS_HITS) || (d_hits && max_ml >= 1)));
  const bool bytes = !(need & K4RS_READS) || (d_reads && d_offs && d_lens);
  const bool segs = !(need & K4RS_SEG2) || d_seg2;
  if (n > 0 && !(records && bytes && segs)) return k4_fail(ix, K4_ERR_PARAMS, "null buffer");
  rs->rr = pe ? nullptr : (k4_read_result*)d_rr;
  rs->hits = pe ? nullptr : (k4_hit*)d_hits;
  rs->max_ml = (int)max_ml;
  rs->pr = pe ? (k4_pe_read*)d_pe : nullptr;
  rs->seg2 = pe ? nullptr : (const k4_seg2*)d_seg2;
  rs->reads = (uint8_t*)d_reads;
  rs->offs = (const uint64_t*)d_offs;
  rs->lens = (const uint32_t*)d_lens;
  rs->n_reads = (pe && (need & K4RS_UNITS)) ? 2 * n : n;
  return K4_OK;
}

// rocPRIM's two calls (K4Scratch, the temporary, is in k4_pool.h): `call(tmp, bytes)` is the rocPRIM function with the rest of its arguments bound; a null tmp asks for the size
template <typename B, typename F>
int k4s_two_calls(k4_index* ix, const char* what, F call, K4Scratch<B>* keep = nullptr, bool size_only = false) {
  K4Scratch<B> own;
  K4Scratch<B>& s = keep ? *keep : own;
  size_t tb = 0;
  K4_TRY(k4_check_hip(ix, call((void*)nullptr, tb), what));
  if (!s.buf.p || tb > s.bytes) {
    K4_TRY(k4_check_hip(ix, s.buf.alloc(tb), what));
    s.bytes = tb;
  }
  return size_only ? K4_OK : k4_check_hip(ix, call(s.buf.p, tb), what);
}

// out[0 .. *d_count) = the items of in[0 .. n) that pred accepts, in order; *d_count is a 64-bit device word
template <typename B, typename In, typename Out, typename Pred>
int k4s_select(k4_index* ix, In in, Out out, uint64_t* d_count, size_t n, Pred pred, hipStream_t st) {
  return k4s_two_calls<B>(ix, "rocprim::select", [&](void* t, size_t& tb) { return rocprim::select(t, tb, in, out, d_count, n, pred, st); });
}

// stable LSD sorts on the key bits [begin_bit, end_bit); the sorted side is current() afterwards
template <typename B, typename K, typename V>
int k4s_sort_pairs(k4_index* ix, rocprim::double_buffer<K>& keys, rocprim::double_buffer<V>& vals, size_t n, unsigned begin_bit,
                   unsigned end_bit, hipStream_t st) {
  return k4s_two_calls<B>(ix, "rocprim::radix_sort_pairs",
                          [&](void* t, size_t& tb) { return rocprim::radix_sort_pairs(t, tb, keys, vals, n, begin_bit, end_bit, st); });
}
template <typename B, typename K>
int k4s_sort_keys(k4_index* ix, rocprim::double_buffer<K>& keys, size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t st) {
  return k4s_two_calls<B>(ix, "rocprim::radix_sort_keys",
                          [&](void* t, size_t& tb) { return rocprim::radix_sort_keys(t, tb, keys, n, begin_bit, end_bit, st); });
}

// keep: the caller's temporary, which grows to what a call asks for and stays with the caller; size_only: it is made ready for
// this call and nothing runs (k4_snp.hip sizes it for its longest sequence once and scans every sequence with it)
template <typename B, typename In, typename Out, typename Init, typename Op>
int k4s_exclusive_scan(k4_index* ix, In in, Out out, Init init, size_t n, Op op, hipStream_t st, K4Scratch<B>* keep = nullptr,
                       bool size_only = false) {
  return k4s_two_calls<B>(
      ix, "rocprim::exclusive_scan", [&](void* t, size_t& tb) { return rocprim::exclusive_scan(t, tb, in, out, init, n, op, st); }, keep,
      size_only);
}
template <typename B, typename In, typename Out, typename Op>
int k4s_inclusive_scan(k4_index* ix, In in, Out out, size_t n, Op op, hipStream_t st) {
  return k4s_two_calls<B>(ix, "rocprim::inclusive_scan", [&](void* t, size_t& tb) { return rocprim::inclusive_scan(t, tb, in, out, n, op, st); });
}

// The opener of a stage: idx = the i in [0, n) that pred accepts, ascending, *m = how many (on the host: the stream is waited
// for).  idx gets n * 4 bytes for the list and, behind them, the word rocPRIM counts in.
template <typename B, typename Pred>
int k4s_select_indices(k4_index* ix, B& idx, size_t n, Pred pred, hipStream_t st, uint64_t* m) {
  const size_t list = (n * 4 + 7) & ~(size_t)7;
  K4_HIP(ix, idx.alloc(list + 8));
  uint64_t* d_m = reinterpret_cast<uint64_t*>(idx.template as<char>() + list);
  K4_TRY(k4s_select<B>(ix, rocprim::counting_iterator<uint32_t>(0), idx.template as<uint32_t>(), d_m, n, pred, st));
  return k4s_read_back(ix, m, d_m, st);
}
