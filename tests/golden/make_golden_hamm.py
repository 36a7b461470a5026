"""Writes tests/golden/hamm_index.sfx.xz, tests/golden/hamm_cases.xz, tests/golden/hamm_<run>.xz and tests/golden/hamm_<run>.csv.xz
(hamm_<run>.dist.json for a sampled run, for which the front end writes no file: the distribution of its log):
what the reference's own CSfxArray::LocateSfxHammings / LocateHammings return for the crafted spans of tests/hamm_craft.py, and
what `ngskit4b hammings -m0` writes over the same index.  Needs the reference's sources, oracle/_ref/libk4ref.so and
oracle/_ref/ngskit4b (make -C oracle ref ngskit4b); run from the repository root:
  python tests/golden/make_golden_hamm.py [reference root]

The shim below is compiled into a temporary directory against the reference's headers and linked with libk4ref.so; nothing
compiled is kept.  hamm_cases.xz is an xz-compressed .npz: names, and per case i the bytes the call left in a 0xFF-filled array of
the span's length (out_<i>) and its return code (rc[i]).  hamm_<run>.xz holds the byte array over all entries that the engine
calls fill when the spans are cut as RestrictedHammingThread cuts them; hamm_<run>.csv.xz the front end's own report.
"""
import ctypes as C
import io
import json
import lzma
import os
import re
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
extern "C" int k4h_open(const char* sfx) {
  g = new CSfxArray;
  if (g->Open((char*)sfx, false, false, false) != eBSFSuccess || g->SetTargBlock(1) < 0) { delete g; g = nullptr; return -1; }
  return 0;
}
extern "C" void k4h_close() { delete g; g = nullptr; }
extern "C" int k4h_sfx(int rhamm, int both, int klen, int nth, int span_len, uint32_t mn, uint32_t mx, uint32_t entry, uint32_t loci, int iib,
                       uint8_t* out) {
  std::vector<tsIdentNode> nodes(1000);
  return g->LocateSfxHammings(rhamm, both != 0, klen, nth, span_len, mn, mx, entry, loci, iib, out, (int)nodes.size(), nodes.data());
}
extern "C" int k4h_seq(int rhamm, int both, int klen, int nth, int len, uint32_t mn, uint32_t mx, const uint8_t* seq, int iib, uint8_t* out) {
  std::vector<tsIdentNode> nodes(1000);
  std::vector<uint8_t> s(seq, seq + len);
  s.resize(s.size() + 8);
  return g->LocateHammings(rhamm, both != 0, klen, nth, len, mn, mx, s.data(), 0, 0, iib, out, (int)nodes.size(), nodes.data());
}
"""


def _xz(path, data):
    with lzma.open(path, "wb", preset=9) as f:
        f.write(data)


def main():
    import hamm_craft as hc
    import kit4b_amd
    from oracle_bindings import Ref

    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    ref_so = os.path.join(ref_dir, "libk4ref.so")
    names, ts = hc.targets()
    with tempfile.TemporaryDirectory() as tmp:
        src, so, sfx = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libshim.so"), os.path.join(tmp, "hamm_index.sfx")
        open(src, "w").write(SHIM)
        subprocess.check_call(["g++", "-std=gnu++17", "-O1", "-w", "-fpermissive", "-fPIC", "-shared", "-I" + ref_root, "-I" + os.path.join(ref_root, "libkit4b"),
                               "-o", so, src, ref_so, "-Wl,-rpath," + ref_dir])
        Ref().build_sfx(sfx, names, ts, dataset="hamm")
        _xz(os.path.join(HERE, "hamm_index.sfx.xz"), open(sfx, "rb").read())
        L = C.CDLL(so)
        L.k4h_sfx.argtypes = [C.c_int] * 5 + [C.c_uint32] * 4 + [C.c_int, C.c_void_p]
        L.k4h_seq.argtypes = [C.c_int] * 5 + [C.c_uint32] * 2 + [C.c_void_p, C.c_int, C.c_void_p]
        assert L.k4h_open(sfx.encode()) == 0
        arrays, rcs = {}, []
        cases = hc.cases()
        for i, (name, form, what, p, expect) in enumerate(cases):
            rhamm, both, nth, mn, mx, iib = p
            if form == "sfx":
                out = np.full(what[2], 0xFF, dtype=np.uint8)
                rc = L.k4h_sfx(rhamm, both, hc.K, nth, what[2], mn, mx, what[0], what[1], iib, out.ctypes.data)
            else:
                q = np.ascontiguousarray(what, dtype=np.uint8)
                out = np.full(len(q), 0xFF, dtype=np.uint8)
                rc = L.k4h_seq(rhamm, both, hc.K, nth, len(q), mn, mx, q.ctypes.data, iib, out.ctypes.data)
            arrays["out_%d" % i] = out
            rcs.append(rc)
            print(name, rc, out[:8].tolist())
        buf = io.BytesIO()
        np.savez(buf, names=np.array([c[0] for c in cases]), rc=np.array(rcs, dtype=np.int32), **arrays)
        _xz(os.path.join(HERE, "hamm_cases.xz"), buf.getvalue())
        lens = [len(t) for t in ts]
        for run, kw in hc.CSV_RUNS:
            klen, rhamm, nth = kw["kmer_len"], kw["rhamm"], kw.get("sample_nth", 1)
            both, iib = 1 if kw.get("both_strands") else 0, kw.get("intra_inter_both", 0)
            mn, mx = kit4b_amd.HAMMING_DEPTHS[1]
            out = np.full(sum(lens), 0xFF, dtype=np.uint8)
            for eid, loci, sl, oo in zip(*kit4b_amd.hamming_spans(lens, klen)):
                rc = L.k4h_sfx(rhamm, both, klen, nth, int(sl), mn, mx, int(eid), int(loci), iib, out.ctypes.data + int(oo))
                assert rc == 0
            _xz(os.path.join(HERE, run + ".xz"), out.tobytes())
            csv, log = os.path.join(tmp, run + ".csv"), os.path.join(tmp, run + ".log")
            cmd = [os.path.join(ref_dir, "ngskit4b"), "hammings", "-m0", "-s0", "-S0", "-K%d" % klen, "-r%d" % rhamm, "-k%d" % nth, "-z%d" % iib,
                   "-T4", "-i", sfx, "-F", log] + (["-c"] if both else []) + (["-o", csv] if nth == 1 else [])
            subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
            if nth == 1:
                _xz(os.path.join(HERE, run + ".csv.xz"), open(csv, "rb").read())
            else:  # the front end writes no file when it samples: its log's distribution is what it leaves
                text = open(log).read()
                m = re.search(r"Sampled (\d+) K-mers, did not sample (\d+)", text)
                counts = [int(v) for v in re.findall(r"^\s*\d+[ +],(\d+),", text[text.index("EditDist,Freq,Proportion"):], flags=re.M)]
                json.dump(dict(sampled=int(m.group(1)), unsampled=int(m.group(2)), counts=counts[:rhamm + 2]),
                          open(os.path.join(HERE, run + ".dist.json"), "w"))
            print(run, "done")
        L.k4h_close()


if __name__ == "__main__":
    main()
