"""Times SfxIndex.blitz (LocateQuerySeqs, k4_query.hip, then the path stage, k4_blitz.hip, the nodes staying on the device) on a
GPU over tools/query_bench.py's two workloads: synthetic targets, queries that are 1 kb and 10 kb copies of them with 2 %
substitutions.  Prints one JSON line: per workload the device time of the locate and of the path stage, each the best of
--repeats runs behind one warm-up run, their ratio, and the paths per second from the wall clock of the whole call (uploads and
downloads included); --out writes it to a file as well.

The reference's `ngskit4b blitz` is NOT timed here: the figures this tool reports stand alone.

  python tools/blitz_bench.py --mbp 4 --out profiles/blitz_bench.json
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

    assert torch.cuda.is_available(), "blitz_bench needs a GPU"
    rng = np.random.default_rng(20260)
    tlen = int(a.mbp * 1e6 / a.targets)
    ts = [rng.integers(0, 4, tlen).astype(np.uint8) for _ in range(a.targets)]
    cat = np.concatenate([np.concatenate([t, np.array([7], np.uint8)]) for t in ts])
    d_seq = torch.from_numpy(cat).cuda()
    sa = torch.empty(len(cat), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(["t%d" % i for i in range(a.targets)], [tlen] * a.targets),
                                 keep=(sa, d_seq))
    res = dict(tool="blitz_bench", targets=a.targets, target_bp=tlen * a.targets, device=torch.cuda.get_device_name(0), sets=[])
    for qlen, nq in ((1000, 4000), (10000, 400)):
        qs = []
        for _ in range(nq):
            t = ts[int(rng.integers(0, a.targets))]
            s = int(rng.integers(0, tlen - qlen))
            q = t[s:s + qlen].copy()
            pos = rng.choice(qlen, size=qlen // 50, replace=False)
            q[pos] = (q[pos] + rng.integers(1, 4, len(pos))) % 4
            qs.append(q)
        kw = dict(core_len=20, core_delta=10, max_hits=1000, max_iter=100, match_pts=1, mismatch_pts=3, gap_open=5, min_path_score=0,
                  query_len_aligned_pct=75, max_paths=1)
        _, paths, blocks = ix.blitz(qs, **kw)  # warm-up: sizes the workspaces
        wall, locate, path = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            _, paths, blocks = ix.blitz(qs, **kw)
            wall.append(time.perf_counter() - t0)
            locate.append(ix.blitz_ms[0])
            path.append(ix.blitz_ms[1])
        res["sets"].append(dict(query_len=qlen, queries=nq, paths=int(len(paths)), blocks=int(len(blocks)), paths_per_s=round(len(paths) / min(wall), 1),
                                wall_ms=[round(1e3 * w, 2) for w in wall], locate_kernel_ms=[round(d, 3) for d in locate],
                                path_kernel_ms=[round(d, 3) for d in path], path_over_locate=round(min(path) / min(locate), 3), **kw))
    ix.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
