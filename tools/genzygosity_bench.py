"""Times SfxIndex.zygosity (`genzygosity`, kit4b_amd/csrc/k4_zygosity.hip) on a GPU: a synthetic pseudo-genome of --entries sequences
that descend from one random ancestor by --div substitutions per base, each with an (AC)n stretch of --repeat bases so that -m3
sends some windows through the ordered walk.  One warm-up, then --repeats scans over every entry: `kernel_ms` is the time on the
stream from a call's first launch to its last (the host looks at the list of deferred windows once per 1 048 576 start loci, and
that wait is inside it), `wall_ms` the wall clock of the Python call, `ns_per_window` comes from the best kernel time, `ordered_share`
is the share of the windows that took the ordered path and `second_launch` how many of them needed tables in device memory.
Prints one JSON line; --out writes it to a file as well.  No reference time is taken and no threshold is set.

  python tools/genzygosity_bench.py --mbp 1 --out profiles/genzygosity_bench.json
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
    ap.add_argument("--mbp", type=float, default=1.0, help="total length of all entries")
    ap.add_argument("--entries", type=int, default=5)
    ap.add_argument("--div", type=float, default=0.03)
    ap.add_argument("--repeat", type=int, default=600)
    ap.add_argument("--subseq-len", type=int, default=25)
    ap.add_argument("--max-subs", type=int, default=2)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import kit4b_amd as k4

    assert torch.cuda.is_available(), "genzygosity_bench needs a GPU"
    rng = np.random.default_rng(30314)
    tlen = int(a.mbp * 1e6 / a.entries)
    anc = rng.integers(0, 4, tlen).astype(np.uint8)
    ts = []
    for c in range(a.entries):
        t = anc.copy()
        pos = rng.choice(tlen, size=int(a.div * tlen), replace=False)
        t[pos] = (t[pos] + rng.integers(1, 4, len(pos))) % 4
        at = int(rng.integers(0, tlen - a.repeat))
        t[at:at + a.repeat] = np.tile(np.array([0, 1], np.uint8), a.repeat // 2 + 1)[:a.repeat]
        ts.append(t)
    cat = np.concatenate([np.concatenate([t, np.array([7], np.uint8)]) for t in ts])
    d_seq = torch.from_numpy(cat).cuda()
    sa = torch.empty(len(cat), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr())
    names = ["ent%d" % i for i in range(a.entries)]
    ix = k4.SfxIndex.from_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(names, [tlen] * a.entries), keep=(sa, d_seq))
    res = dict(tool="genzygosity_bench", entries=a.entries, total_bp=tlen * a.entries, divergence=a.div, repeat_bases=a.repeat, subseq_len=a.subseq_len,
               max_subs=a.max_subs, mode=a.mode, device=torch.cuda.get_device_name(0), reference_time="not taken")
    kw = dict(subseq_len=a.subseq_len, max_subs=a.max_subs, mode=a.mode)
    matrix, subseqs, tot = ix.zygosity(**kw)  # warm-up: sizes the workspace
    wall, dev = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        matrix, subseqs, tot = ix.zygosity(**kw)
        wall.append(time.perf_counter() - t0)
        dev.append(ix.zygosity_kernel_ms())
    res.update(totals=tot, subseqs=subseqs.tolist(), wall_ms=[round(1e3 * w, 2) for w in wall], kernel_ms=[round(d, 3) for d in dev],
               ns_per_window=round(1e6 * min(dev) / max(tot["windows"], 1), 2), ordered_share=round(tot["ordered"] / max(tot["windows"], 1), 6),
               second_launch=tot["second_launch"])
    ix.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
