"""Writes tests/golden/kmarkers_index.sfx.xz, tests/golden/kmarkers_calls.xz and tests/golden/kmarkers_<case>.fa.xz: what the
reference's own CSfxArray::IterateExacts (walked to exhaustion) and both CSfxArray::MatchesOtherChroms overloads return for the
probes of tests/kmarkers_craft.py, and the files `ngskit4b kmarkers -T1` writes over the same index for its file cases.  Needs the
reference's sources, oracle/_ref/libk4ref.so and oracle/_ref/ngskit4b (make -C oracle ref ngskit4b); run from the repository root:
  python tests/golden/make_golden_kmarkers.py <reference root>

The shim below is compiled into a temporary directory against the reference's headers and linked with libk4ref.so; nothing
compiled is kept.  The front end sleeps ten seconds in every run; the runs go side by side.  kmarkers_calls.xz is an xz-compressed
.npz: the probes (cat / offs / lens), per probe the id list (ids_cat / ids_offs) and MaxTotMM (mm), the walk (walk_offs into
walk_idx / walk_entry / walk_loci; walk_idx holds IterateExacts' return values), m1 = MatchesOtherChroms(ids[0], ..) and
mn = MatchesOtherChroms(len(ids), ids, ..)."""
import concurrent.futures
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

SHIM = r"""
#include "libkit4b/commhdrs.h"
static CSfxArray* g = nullptr;
extern "C" int k4m_open(const char* sfx) {
  g = new CSfxArray;
  if (g->Open((char*)sfx, false, false, false) != eBSFSuccess || g->SetTargBlock(1) < 0) { delete g; g = nullptr; return -1; }
  return 0;
}
extern "C" void k4m_close() { delete g; g = nullptr; }
extern "C" int64_t k4m_iterate(uint8_t* probe, uint32_t len, int64_t prev, uint32_t* entry, uint32_t* loci) {
  return g->IterateExacts(probe, len, prev, entry, loci);
}
extern "C" int k4m_match1(int id, int mm, int len, uint8_t* probe) { return g->MatchesOtherChroms(id, mm, len, probe); }
extern "C" int k4m_matchn(int n, int* ids, int mm, int len, uint8_t* probe) { return g->MatchesOtherChroms(n, ids, mm, len, probe); }
"""


def _xz(path, data):
    with lzma.open(path, "wb", preset=9) as f:
        f.write(data)


def front_end_args(kw):
    a = ["-m%d" % kw.get("mode", 0), "-k%d" % kw["kmer_len"]]
    if "prefix_len" in kw:
        a.append("-p%d" % kw["prefix_len"])
    if "min_shared" in kw:
        a.append("-s%d" % kw["min_shared"])
    if "min_hamming" in kw:
        a.append("-K%d" % kw["min_hamming"])
    return a


def main():
    import kmarkers_craft as kc
    from oracle_bindings import Ref

    ref_root = sys.argv[1]
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    ref_so = os.path.join(ref_dir, "libk4ref.so")
    names, seqs, _ = kc.build()
    with tempfile.TemporaryDirectory() as tmp:
        src, so, sfx = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libshim.so"), os.path.join(tmp, "kmarkers_index.sfx")
        open(src, "w").write(SHIM)
        subprocess.check_call(["g++", "-std=gnu++17", "-O1", "-w", "-fpermissive", "-fPIC", "-shared", "-I" + ref_root, "-I" + os.path.join(ref_root, "libkit4b"),
                               "-o", so, src, ref_so, "-Wl,-rpath," + ref_dir])
        Ref().build_sfx(sfx, names, seqs, dataset="kmarkers")
        _xz(os.path.join(HERE, "kmarkers_index.sfx.xz"), open(sfx, "rb").read())

        def front_end(case):
            stem, kw = case
            fa, log = os.path.join(tmp, stem + ".fa"), os.path.join(tmp, stem + ".log")
            cmd = [os.path.join(ref_dir, "ngskit4b"), "kmarkers"] + front_end_args(kw) + ["-c", kc.CULTIVAR, "-C", ",".join(kc.TARGET_NAMES), "-T1",
                                                                                          "-i", sfx, "-o", fa, "-F", log]
            subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
            return stem, open(fa, "rb").read()

        with concurrent.futures.ThreadPoolExecutor(8) as pool:
            runs = pool.map(front_end, kc.file_cases())
            L = C.CDLL(so)
            L.k4m_iterate.restype = C.c_int64
            L.k4m_iterate.argtypes = [C.c_void_p, C.c_uint32, C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
            L.k4m_match1.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
            L.k4m_matchn.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            assert L.k4m_open(sfx.encode()) == 0
            pr = kc.probes(seqs)
            walk_offs, w_idx, w_ent, w_loci, m1, mn = [0], [], [], [], [], []
            for s, ids, mm in pr:
                buf = np.ascontiguousarray(s, dtype=np.uint8)
                prev, e, l = 0, C.c_uint32(0), C.c_uint32(0)
                while True:
                    nxt = L.k4m_iterate(buf.ctypes.data, len(buf), prev, C.byref(e), C.byref(l))
                    if nxt <= 0:
                        break
                    w_idx.append(nxt); w_ent.append(e.value); w_loci.append(l.value)
                    prev = nxt
                walk_offs.append(len(w_idx))
                a = np.array(ids, dtype=np.int32)
                m1.append(L.k4m_match1(int(ids[0]), mm, len(buf), buf.ctypes.data))
                mn.append(L.k4m_matchn(len(a), a.ctypes.data, mm, len(buf), buf.ctypes.data))
            L.k4m_close()
            lens = np.array([len(p[0]) for p in pr], dtype=np.uint32)
            id_lens = [len(p[1]) for p in pr]
            out = io.BytesIO()
            np.savez(out, cat=np.concatenate([p[0] for p in pr]).astype(np.uint8), lens=lens,
                     offs=np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64),
                     ids_cat=np.concatenate([np.array(p[1], dtype=np.uint32) for p in pr]), ids_offs=np.concatenate([[0], np.cumsum(id_lens)]).astype(np.int64),
                     mm=np.array([p[2] for p in pr], dtype=np.int32), walk_offs=np.array(walk_offs, dtype=np.int64), walk_idx=np.array(w_idx, dtype=np.int64),
                     walk_entry=np.array(w_ent, dtype=np.uint32), walk_loci=np.array(w_loci, dtype=np.uint32), m1=np.array(m1, dtype=np.int32),
                     mn=np.array(mn, dtype=np.int32))
            _xz(os.path.join(HERE, "kmarkers_calls.xz"), out.getvalue())
            print("probes", len(pr), "hits", len(w_idx), "m1", sum(m1), "mn", sum(mn))
            for stem, data in runs:
                _xz(os.path.join(HERE, stem + ".fa.xz"), data)
                print(stem, len(data), data[:40])


if __name__ == "__main__":
    main()
