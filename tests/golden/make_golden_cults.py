"""Writes tests/golden/cults_index.sfx.xz, tests/golden/cults_cases.xz and tests/golden/cults_<run>.fa.xz: what the reference's own
CSfxArray::GenKMerCultsCnts / GenKMerCultThreadRange hand to a recording callback and return for the cases of tests/cults_craft.py,
and what `ngskit4b prekmarkers -T1 -S0` (kmermarkers.cpp; the front end lists it under that name) writes over the same index.  Needs the reference's sources, oracle/_ref/libk4ref.so and
oracle/_ref/ngskit4b (make -C oracle ref ngskit4b); run from the repository root:
  python tests/golden/make_golden_cults.py [reference root]

The shim below is compiled into a temporary directory against the reference's headers and linked with libk4ref.so; nothing
compiled is kept.  cults_cases.xz is an xz-compressed .npz: names, rc[i], start[i] / end[i] (the range the case resolved to; -1 for a
thread the partition leaves nothing), and per case the callbacks as bytes (cb_<i>, see parse_callbacks in test_cults_cpu.py);
tr_rc / tr_end the thread ranges; abort_rc / abort_cb a run whose third callback answers -7.
"""
import ctypes as C
import io
import lzma
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

RUNS = [("cults_k20", dict(kmer_len=20)), ("cults_k24_p20_s2", dict(kmer_len=24, prefix_len=20, min_shared=2)),
        ("cults_k20_sense_s1", dict(kmer_len=20, min_shared=1, sense_only=True))]

SHIM = r"""
#include "libkit4b/commhdrs.h"
static CSfxArray* g = nullptr;
static std::vector<uint8_t> rec;
static int klen = 0, n_cb = 0, abort_at = 0;
extern "C" int k4c_open(const char* sfx) {
  g = new CSfxArray;
  if (g->Open((char*)sfx, false, false, false) != eBSFSuccess || g->SetTargBlock(1) < 0) { delete g; g = nullptr; return -1; }
  return 0;
}
extern "C" void k4c_close() { delete g; g = nullptr; }
template <typename T> static void put(T v) { const uint8_t* p = (const uint8_t*)&v; rec.insert(rec.end(), p, p + sizeof(T)); }
// a callback as bytes: sense u64, antisense u64, NumCultivars u32, TotCultivars u32, dense layout as expected u32, entries with a
// count u32, KMerSeq (K + 1 bytes), then {EntryID, SenseCnts, AntisenseCnts} u32 x 3 of those entries in table order
static int record(void*, tsKMerCultsCnts* p) {
  uint32_t nnz = 0, dense_ok = 1;
  for (uint32_t i = 0; i < (uint32_t)cMaxCultivars; i++) {
    const tsKMerCultDist& d = p->CultCnts[i];
    if (i < p->TotCultivars) { if (d.EntryID != i + 1) dense_ok = 0; if (d.SenseCnts || d.AntisenseCnts) nnz++; }
    else if (d.EntryID || d.SenseCnts || d.AntisenseCnts) dense_ok = 0;
  }
  put<uint64_t>(p->SenseCnts); put<uint64_t>(p->AntisenseCnts); put<uint32_t>(p->NumCultivars); put<uint32_t>(p->TotCultivars);
  put<uint32_t>(dense_ok); put<uint32_t>(nnz);
  rec.insert(rec.end(), p->KMerSeq, p->KMerSeq + klen + 1);
  for (uint32_t i = 0; i < p->TotCultivars; i++) {
    const tsKMerCultDist& d = p->CultCnts[i];
    if (d.SenseCnts || d.AntisenseCnts) { put<uint32_t>(d.EntryID); put<uint32_t>(d.SenseCnts); put<uint32_t>(d.AntisenseCnts); }
  }
  return ++n_cb == abort_at ? -7 : 0;
}
extern "C" int64_t k4c_cults(int sense_only, int64_t start, int64_t end, int plen, int slen, int min_cult, int max_homo, int abort_after) {
  rec.clear(); klen = plen + slen; n_cb = 0; abort_at = abort_after;
  return g->GenKMerCultsCnts(sense_only != 0, start, end, plen, slen, min_cult, max_homo, nullptr, record);
}
extern "C" uint64_t k4c_bytes() { return rec.size(); }
extern "C" void k4c_copy(uint8_t* out) { memcpy(out, rec.data(), rec.size()); }
extern "C" int k4c_range(int klen_, int inst, int nthreads, int64_t start, int64_t* end) { return g->GenKMerCultThreadRange(klen_, inst, nthreads, start, end); }
"""


def _xz(path, data):
    with lzma.open(path, "wb", preset=9) as f:
        f.write(data)


def main():
    import cults_craft as cc
    import cults_ref
    import query_ref
    from oracle_bindings import Oracle, Ref

    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    ref_so = os.path.join(ref_dir, "libk4ref.so")
    names, ts = cc.targets()
    with tempfile.TemporaryDirectory() as tmp:
        src, so, sfx = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libshim.so"), os.path.join(tmp, "cults_index.sfx")
        open(src, "w").write(SHIM)
        subprocess.check_call(["g++", "-std=gnu++17", "-O1", "-w", "-fpermissive", "-fPIC", "-shared", "-I" + ref_root, "-I" + os.path.join(ref_root, "libkit4b"),
                               "-o", so, src, ref_so, "-Wl,-rpath," + ref_dir])
        Ref().build_sfx(sfx, names, ts, dataset="cults")
        _xz(os.path.join(HERE, "cults_index.sfx.xz"), open(sfx, "rb").read())
        O = Oracle()
        h = O.open(sfx)
        index = query_ref.index_from_oracle(O, h)
        L = C.CDLL(so)
        L.k4c_cults.restype = C.c_int64
        L.k4c_cults.argtypes = [C.c_int, C.c_int64, C.c_int64] + [C.c_int] * 5
        L.k4c_bytes.restype = C.c_uint64
        L.k4c_copy.argtypes = [C.c_void_p]
        L.k4c_range.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int64)]
        assert L.k4c_open(sfx.encode()) == 0

        def ref_range(_, klen, inst, nt, start):
            e = C.c_int64(0)
            return L.k4c_range(klen, inst, nt, start, C.byref(e)), e.value

        def run(kw, rng, abort_after=0):
            rc = L.k4c_cults(1 if kw["sense_only"] else 0, rng[0], rng[1], kw["plen"], kw["slen"], kw["min_cult"], kw["max_homo"], abort_after)
            out = np.zeros(L.k4c_bytes(), dtype=np.uint8)
            if len(out):
                L.k4c_copy(out.ctypes.data)
            return rc, out

        arrays, rcs, starts, ends, tr_rc, tr_end = {}, [], [], [], [], []
        cases = cc.cases()
        for i, (name, kw, rng) in enumerate(cases):
            if isinstance(rng, tuple) and rng[0] == "thread":
                start = 0
                for t in range(1, rng[2] + 1):
                    trc, tend = ref_range(None, cc.P, t, rng[1], start)
                    if t < rng[2] and trc >= 1:
                        start = tend + 1
                tr_rc.append(trc)
                tr_end.append(tend)
            r = cc.resolve(rng, index, ref_range)
            if r is None or (name == "homozygotic_unsupported"):
                rc, out, r = (0, np.zeros(0, np.uint8), r or (-1, -1)) if r is None else (-3, np.zeros(0, np.uint8), r)
            else:
                rc, out = run(kw, r)
            arrays["cb_%d" % i] = out
            rcs.append(rc)
            starts.append(r[0])
            ends.append(r[1])
            print(name, r, rc, len(out))
        abort_rc, abort_cb = run(cases[2][1], (0, 0), 3)
        buf = io.BytesIO()
        np.savez(buf, names=np.array([c[0] for c in cases]), rc=np.array(rcs, dtype=np.int64), start=np.array(starts, dtype=np.int64),
                 end=np.array(ends, dtype=np.int64), tr_rc=np.array(tr_rc, dtype=np.int64), tr_end=np.array(tr_end, dtype=np.int64),
                 abort_rc=np.array([abort_rc], dtype=np.int64), abort_cb=abort_cb, **arrays)
        _xz(os.path.join(HERE, "cults_cases.xz"), buf.getvalue())
        for run_name, kw in RUNS:
            fa, log = os.path.join(tmp, run_name + ".fa"), os.path.join(tmp, run_name + ".log")
            cmd = [os.path.join(ref_dir, "ngskit4b"), "prekmarkers", "-m%d" % (1 if kw.get("sense_only") else 0), "-k%d" % kw["kmer_len"],
                   "-p%d" % kw.get("prefix_len", kw["kmer_len"]), "-s%d" % kw.get("min_shared", 0), "-S0", "-T1", "-i", sfx, "-o", fa, "-F", log]
            subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
            _xz(os.path.join(HERE, run_name + ".fa.xz"), open(fa, "rb").read())
            print(run_name, "done", os.path.getsize(fa))
        L.k4c_close()
        O.close(h)
        big(tmp, ref_dir, L, O)


def big(tmp, ref_dir, L, O):
    """tests/golden/cults_big.xz and cults_big_k20_T4.fa.xz: the thread ranges of 2, 3 and 4 threads over cults_craft.big_targets(), the
    callbacks of four and of three threads over their ranges (MinCultivars 0, in range order: cb_all4 / cb_all3, located4 / located3),
    per boundary of the three the callbacks of the 150 elements up to it and of the 150 behind it (MinCultivars 1: win_rc, win_<k>;
    each of these boundaries cuts a K-mer off its other elements), and the front end's file
    with -T4.  The index itself is not kept: the tests build it, and the suffix array the project's builder gives is checked
    here to hold the reference's text at every place."""
    import cults_craft as cc
    import query_ref
    from oracle_bindings import Ref

    names, ts = cc.big_targets()
    sfx = os.path.join(tmp, "cults_big.sfx")
    Ref().build_sfx(sfx, names, ts, dataset="cultsbig")
    h = O.open(sfx)
    index = query_ref.index_from_oracle(O, h)
    O.close(h)
    h2 = O.build(names, ts, dataset="cultsbig", threads=4)
    own = query_ref.index_from_oracle(O, h2)
    O.close(h2)
    # (the two builders may order suffixes that are equal up to their end-of-sequence symbol differently: the same text stands at
    # every place of the array, which is all the sweep and the thread ranges look at)
    assert own[0] == index[0] and own[2] == index[2] and len(own[1]) == len(index[1])
    for x, y in zip(own[1], index[1]):
        if x != y:
            e = index[0].index(7, x)  # (eBaseEOS)
            assert index[0][x:e + 1] == index[0][y:y + e + 1 - x], (x, y)
    assert L.k4c_open(sfx.encode()) == 0

    def ref_range(_, klen, inst, nt, start):
        e = C.c_int64(0)
        return L.k4c_range(klen, inst, nt, start, C.byref(e)), e.value

    def run(start, end, min_cult):
        rc = L.k4c_cults(0, start, end, cc.P, cc.S, min_cult, 0, 0)
        out = np.zeros(L.k4c_bytes(), dtype=np.uint8)
        if len(out):
            L.k4c_copy(out.ctypes.data)
        return rc, out

    tr = [(nt,) + row for nt in cc.BIG_THREADS for row in cc.thread_ranges(index, ref_range, nt)]
    four, three = [r for r in tr if r[0] == 4], [r for r in tr if r[0] == 3]
    assert len(four) == 4 and all(r[3] == 1 for r in four) and len(three) == 3
    arrays, win_rc = {}, []
    for key, rows in (("4", four), ("3", three)):
        located, blobs = [], []
        for _, t, start, rc, end in rows:
            n, out = run(start, end, 0)
            located.append(n)
            blobs.append(out)
        arrays["located" + key], arrays["cb_all" + key] = np.array(located, dtype=np.int64), np.concatenate(blobs)
    for k, (_, t, start, rc, end) in enumerate(three[:2]):
        for j, (a, b) in enumerate(((end - 150, end), (end + 1, end + 150))):
            n, out = run(a, b, 1)
            win_rc.append(n)
            arrays["win_%d" % (2 * k + j)] = out
    buf = io.BytesIO()
    np.savez(buf, tr=np.array(tr, dtype=np.int64), win_rc=np.array(win_rc, dtype=np.int64), **arrays)
    _xz(os.path.join(HERE, "cults_big.xz"), buf.getvalue())
    fa = os.path.join(tmp, "big.fa")
    subprocess.check_call([os.path.join(ref_dir, "ngskit4b"), "prekmarkers", "-m0", "-k20", "-p20", "-s0", "-S0", "-T4", "-i", sfx, "-o", fa, "-F",
                           os.path.join(tmp, "big.log")], stdout=subprocess.DEVNULL)
    _xz(os.path.join(HERE, "cults_big_k20_T4.fa.xz"), open(fa, "rb").read())
    print("big", tr, win_rc, os.path.getsize(fa))
    L.k4c_close()


if __name__ == "__main__":
    main()
