"""Writes tests/golden/zygosity_index.sfx.xz, tests/golden/zygosity_calls.xz and tests/golden/zygosity_<case>[_raw].csv.xz: what the
reference's own CSfxArray::LocateAllNearMatches returns for the calls of tests/zyg_craft.py, and the two files `genzygosity -o -O`
writes over the same index for its four runs (each run with -T1 and with -T4, which must agree).  Needs the reference's sources,
oracle/_ref/libk4ref.so and the archives under oracle/_ref/ngs (make -C oracle ref ngskit4b); run from the repository root:
  python tests/golden/make_golden_zygosity.py <reference root>

The shim below and genzygosity itself are compiled into a temporary directory; nothing compiled is kept.  zygosity_calls.xz is an
xz-compressed .npz: the probes (cat / offs / lens), per call the columns of zyg_craft.calls(), rslt, and cnt_offs into cnt (the
NumEntries counts of every call, as the reference left them)."""
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

COLS = ("probe_entry", "probe_ofs", "max_tot_mm", "core_len", "core_delta", "max_core_slides", "max_matches", "num_entries", "cur_max_iter",
        "n_ident_nodes")

SHIM = r"""
#include "libkit4b/commhdrs.h"
static CSfxArray* g = nullptr;
static tsIdentNode* nodes = nullptr;
extern "C" int k4z_open(const char* sfx) {
  g = new CSfxArray;
  if (g->Open((char*)sfx, false, false, false) != eBSFSuccess || g->SetTargBlock(1) < 0) { delete g; g = nullptr; return -1; }
  nodes = new tsIdentNode[1024000];
  return 0;
}
extern "C" void k4z_close() { delete g; g = nullptr; delete[] nodes; }
extern "C" int k4z_near(int mm, int core_len, int core_delta, int slides, int max_matches, int num_entries, uint32_t* counts, uint32_t entry,
                        uint32_t ofs, int len, uint8_t* probe, int max_iter, int n_nodes) {
  return g->LocateAllNearMatches(mm, core_len, core_delta, slides, max_matches, num_entries, counts, entry, ofs, len, probe, max_iter, n_nodes, nodes);
}
"""


def _xz(path, data):
    with lzma.open(path, "wb", preset=9 | lzma.PRESET_EXTREME) as f:
        f.write(data)


def main():
    import zyg_craft as zc
    from oracle_bindings import Oracle

    ref_root = sys.argv[1]
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    ref_so = os.path.join(ref_dir, "libk4ref.so")
    names, seqs, sites = zc.build()
    with tempfile.TemporaryDirectory() as tmp:
        src, so, sfx, exe = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libshim.so"), os.path.join(tmp, "zygosity_index.sfx"), os.path.join(tmp, "genzygosity")
        open(src, "w").write(SHIM)
        flags = ["-std=gnu++17", "-O1", "-w", "-fpermissive", "-I" + ref_root, "-I" + os.path.join(ref_root, "libkit4b")]
        subprocess.check_call(["g++"] + flags + ["-fPIC", "-shared", "-o", so, src, ref_so, "-Wl,-rpath," + ref_dir])
        ngs = os.path.join(ref_dir, "ngs")
        subprocess.check_call(["g++"] + flags + ["-I" + os.path.join(ref_root, "genzygosity"), "-o", exe, os.path.join(ref_root, "genzygosity", "genzygosity.cpp"),
                                                 os.path.join(ngs, "libkit4b.a"), os.path.join(ngs, "libz.a"), "-lrt", "-ldl", "-lpthread"])
        O = Oracle()
        h = O.build(names, seqs, dataset="zygosity", threads=4)
        O.write(h, sfx)
        O.close(h)
        _xz(os.path.join(HERE, "zygosity_index.sfx.xz"), open(sfx, "rb").read())

        def front_end(job):
            (stem, kw), threads = job
            o, r, log = (os.path.join(tmp, "%s_T%d.%s" % (stem, threads, x)) for x in ("csv", "raw", "log"))
            subprocess.check_call([exe] + zc.front_end_args(kw) + ["-T%d" % threads, "-i", sfx, "-o", o, "-O", r, "-F", log], stdout=subprocess.DEVNULL)
            return stem, threads, open(o, "rb").read(), open(r, "rb").read()

        with concurrent.futures.ThreadPoolExecutor(8) as pool:
            runs = pool.map(front_end, [(c, t) for c in zc.scan_cases() for t in (1, 4)])
            L = C.CDLL(so)
            assert L.k4z_open(sfx.encode()) == 0
            calls = zc.calls(seqs, sites)
            rslt, cnt, cnt_offs = [], [], [0]
            for c in calls:
                buf = np.ascontiguousarray(c["probe"], dtype=np.uint8)
                keep = buf.copy()
                counts = np.full(max(c["num_entries"], 1), 0xEEEEEEEE, dtype=np.uint32)
                rslt.append(L.k4z_near(c["max_tot_mm"], c["core_len"], c["core_delta"], c["max_core_slides"], c["max_matches"], c["num_entries"],
                                       C.c_void_p(counts.ctypes.data), c["probe_entry"], c["probe_ofs"], len(buf), C.c_void_p(buf.ctypes.data),
                                       c["cur_max_iter"], c["n_ident_nodes"]))
                assert np.array_equal(buf, keep)
                cnt.extend(counts[:c["num_entries"]].tolist())
                cnt_offs.append(len(cnt))
            L.k4z_close()
            lens = np.array([len(c["probe"]) for c in calls], dtype=np.uint32)
            out = io.BytesIO()
            np.savez(out, cat=np.concatenate([c["probe"] for c in calls]).astype(np.uint8), lens=lens,
                     offs=np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64), rslt=np.array(rslt, dtype=np.int32),
                     cnt=np.array(cnt, dtype=np.uint32), cnt_offs=np.array(cnt_offs, dtype=np.int64),
                     **{k: np.array([c[k] for c in calls], dtype=np.int32) for k in COLS})
            _xz(os.path.join(HERE, "zygosity_calls.xz"), out.getvalue())
            r = np.array(rslt)
            print("calls", len(calls), "minus one", int((r < 0).sum()), "zero", int((r == 0).sum()), "max", int(r.max()))
            got = {}
            for stem, threads, o, raw in runs:
                got.setdefault(stem, []).append((o, raw))
            for stem, pair in got.items():
                assert pair[0] == pair[1], stem + ": -T1 and -T4 differ"
                _xz(os.path.join(HERE, stem + ".csv.xz"), pair[0][0])
                _xz(os.path.join(HERE, stem + "_raw.csv.xz"), pair[0][1])
                print(stem, len(pair[0][0]), len(pair[0][1]), pair[0][0][:60])


if __name__ == "__main__":
    main()
