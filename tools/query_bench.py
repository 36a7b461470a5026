"""Times k4_locate_query_seqs_batch (LocateQuerySeqs, kit4b_amd/csrc/k4_query.hip) on a GPU: synthetic targets, queries that are
1 kb and 10 kb copies of them with 2 % substitutions.  Prints one JSON line (queries/s from the wall clock of the host-pointer
entry, upload and download included, and the device time of its kernels); --out writes it to a file as well.

The reference's `ngskit4b blitz` is NOT timed here: the figure this tool reports stands alone.

  python tools/query_bench.py --mbp 4 --out profiles/query_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=4.0, help="total target length")
    ap.add_argument("--targets", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import kit4b_amd as k4

    assert torch.cuda.is_available(), "query_bench needs a GPU"
    rng = np.random.default_rng(20260)
    tlen = int(a.mbp * 1e6 / a.targets)
    ts = [rng.integers(0, 4, tlen).astype(np.uint8) for _ in range(a.targets)]
    cat = np.concatenate([np.concatenate([t, np.array([7], np.uint8)]) for t in ts])
    d_seq = torch.from_numpy(cat).cuda()
    sa = torch.empty(len(cat), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(["t%d" % i for i in range(a.targets)], [tlen] * a.targets),
                                 keep=(sa, d_seq))
    res = dict(tool="query_bench", targets=a.targets, target_bp=tlen * a.targets, device=torch.cuda.get_device_name(0), sets=[])
    for qlen, nq in ((1000, 4000), (10000, 400)):
        qs = []
        for _ in range(nq):
            t = ts[int(rng.integers(0, a.targets))]
            s = int(rng.integers(0, tlen - qlen))
            q = t[s:s + qlen].copy()
            pos = rng.choice(qlen, size=qlen // 50, replace=False)
            q[pos] = (q[pos] + rng.integers(1, 4, len(pos))) % 4
            qs.append(q)
        kw = dict(core_len=20, core_delta=10, max_hits=1000, max_iter=100, match_pts=1, mismatch_pts=3)
        nodes = ix.locate_query_seqs(qs, **kw)  # warm-up: sizes the workspace
        wall, dev = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            nodes = ix.locate_query_seqs(qs, nodes_cap=sum(len(n) for n in nodes), **kw)
            wall.append(time.perf_counter() - t0)
            dev.append(ix.query_kernel_ms())
        res["sets"].append(dict(query_len=qlen, queries=nq, nodes=int(sum(len(n) for n in nodes)), queries_per_s=round(nq / min(wall), 1),
                                wall_ms=[round(1e3 * w, 2) for w in wall], kernel_ms=[round(d, 3) for d in dev], **kw))
    ix.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
