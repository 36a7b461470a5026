"""Writes tests/golden/query_index.sfx.xz and tests/golden/query_<group>.xz: what the reference's own CSfxArray::LocateQuerySeqs
returns for the crafted queries of tests/query_craft.py.  Needs the reference's sources and oracle/_ref/libk4ref.so
(make -C oracle ref); run from the repository root:  python tests/golden/make_golden_query.py [reference root]

The shim below is compiled into a temporary directory against the reference's headers and linked with libk4ref.so; nothing
compiled is kept.  One fresh CSfxArray per group: no InitOverOccKMers, no InitKMerCountDists, no InitialiseCoreKMers, one thread.
A fixture is an xz-compressed .npz: cat / offs / lens (the queries), params [n, 7] (query_craft.PARAM_NAMES), names, node_offs
[n + 1] and nodes [m, 7] in query_ref.NODE_FIELDS order.
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

SHIM = r"""
#include "libkit4b/commhdrs.h"
extern "C" int k4q_run(const char* sfx, int n, const uint8_t* cat, const uint64_t* offs, const uint32_t* lens, const int32_t* params,
                       uint32_t* out, uint64_t* node_offs, uint64_t cap) {
  CSfxArray* p = new CSfxArray;
  if (p->Open((char*)sfx, false, false, false) != eBSFSuccess || p->SetTargBlock(1) < 0) { delete p; return -1; }
  uint64_t m = 0;
  for (int i = 0; i < n; i++) {
    const int32_t* q = params + 7 * i;
    std::vector<uint8_t> probe(cat + offs[i], cat + offs[i] + lens[i]);
    probe.resize(probe.size() + 8);
    std::vector<tsQueryAlignNodes> hits((size_t)q[3] + 1);
    node_offs[i] = m;
    int r = p->LocateQuerySeqs((uint32_t)(i + 1), probe.data(), lens[i], (uint32_t)q[0], (uint32_t)q[1], (eALStrand)q[2], (uint32_t)q[3],
                               hits.data(), (uint32_t)q[4], q[5], q[6]);
    if (r < 0 || m + (uint64_t)r > cap) { delete p; return -2; }
    if (memcmp(probe.data(), cat + offs[i], lens[i]) != 0) { delete p; return -3; }  // the probe comes back as it went in
    for (int k = 0; k < r; k++, m++) {
      const tsQueryAlignNodes& h = hits[k];
      if (h.QueryID != i + 1 || h.FlgRedundant || h.HiScore || h.HiScorePathNextIdx) { delete p; return -4; }
      uint32_t* o = out + 7 * m;
      o[0] = h.QueryStartOfs; o[1] = h.AlignLen; o[2] = h.TargSeqID; o[3] = h.TargSeqLoci; o[4] = h.NumMismatches; o[5] = h.AlignNodeID;
      o[6] = h.FlgStrand;
    }
  }
  node_offs[n] = m;
  delete p;
  return 0;
}
"""


def main():
    import query_craft as qc
    from oracle_bindings import Ref

    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libk4ref.so")
    names, ts = qc.targets()
    with tempfile.TemporaryDirectory() as tmp:
        src, so, sfx = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libshim.so"), os.path.join(tmp, "query_index.sfx")
        open(src, "w").write(SHIM)
        subprocess.check_call(["g++", "-std=gnu++17", "-O1", "-w", "-fpermissive", "-fPIC", "-shared", "-I" + ref_root, "-I" + os.path.join(ref_root, "libkit4b"),
                               "-o", so, src, ref_so, "-Wl,-rpath," + os.path.dirname(ref_so)])
        Ref().build_sfx(sfx, names, ts, dataset="query")
        with open(sfx, "rb") as f, lzma.open(os.path.join(HERE, "query_index.sfx.xz"), "wb", preset=9) as g:
            g.write(f.read())
        L = C.CDLL(so)
        L.k4q_run.argtypes = [C.c_char_p, C.c_int] + [C.c_void_p] * 6 + [C.c_uint64]
        for group, cases in qc.groups().items():
            qs = [np.ascontiguousarray(c[1], dtype=np.uint8) for c in cases]
            lens = np.array([len(q) for q in qs], dtype=np.uint32)
            offs = np.zeros(len(qs), dtype=np.uint64)
            offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
            cat = np.concatenate(qs + [np.zeros(16, np.uint8)])
            params = np.array([c[2] for c in cases], dtype=np.int32)
            cap = 1 << 16
            out = np.zeros((cap, 7), dtype=np.uint32)
            node_offs = np.zeros(len(qs) + 1, dtype=np.uint64)
            rc = L.k4q_run(sfx.encode(), len(qs), cat.ctypes.data, offs.ctypes.data, lens.ctypes.data, params.ctypes.data, out.ctypes.data,
                           node_offs.ctypes.data, cap)
            assert rc == 0, (group, rc)
            buf = io.BytesIO()
            np.savez(buf, cat=cat, offs=offs, lens=lens, params=params, names=np.array([c[0] for c in cases]), node_offs=node_offs,
                     nodes=out[:int(node_offs[-1])])
            with lzma.open(os.path.join(HERE, "query_%s.xz" % group), "wb", preset=9) as g:
                g.write(buf.getvalue())
            print(group, len(qs), "queries", int(node_offs[-1]), "nodes", [int(b - a) for a, b in zip(node_offs[:-1], node_offs[1:])])


if __name__ == "__main__":
    main()
