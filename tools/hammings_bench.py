"""Times k4_locate_sfx_hammings_batch (restricted Hammings, kit4b_amd/csrc/k4_hamming.hip) on a GPU: synthetic random targets with
planted copies of 1 kb pieces at 0..4 % divergence, every K-mer of every target (the spans cut as `ngskit4b hammings` cuts them),
K = 100, r = 3, the default depth preset, sense only and both strands.  One warm-up, then the best of --repeats runs.  Prints one
JSON line (K-mers/s from the wall clock of the host-pointer entry, upload and download of the byte array included, and the device
time of its launches); --out writes it to a file as well.

The reference's `ngskit4b hammings` is NOT timed here: the figure this tool reports stands alone, and no threshold is set for it.

  python tools/hammings_bench.py --mbp 4 --out profiles/hammings_bench.json
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
    ap.add_argument("--copies", type=int, default=400, help="planted 1 kb copies")
    ap.add_argument("--kmer-len", type=int, default=100)
    ap.add_argument("--rhamm", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import kit4b_amd as k4

    assert torch.cuda.is_available(), "hammings_bench needs a GPU"
    rng = np.random.default_rng(20261)
    tlen = int(a.mbp * 1e6 / a.targets)
    ts = [rng.integers(0, 4, tlen).astype(np.uint8) for _ in range(a.targets)]
    for c in range(a.copies):  # a 1 kb piece of one target over 1 kb of another place, c % 5 per cent of it substituted
        src, dst = ts[int(rng.integers(0, a.targets))], ts[int(rng.integers(0, a.targets))]
        s, d = int(rng.integers(0, tlen - 1000)), int(rng.integers(0, tlen - 1000))
        piece = src[s:s + 1000].copy()
        pos = rng.choice(1000, size=10 * (c % 5), replace=False)
        piece[pos] = (piece[pos] + rng.integers(1, 4, len(pos))) % 4
        dst[d:d + 1000] = piece
    cat = np.concatenate([np.concatenate([t, np.array([7], np.uint8)]) for t in ts])
    d_seq = torch.from_numpy(cat).cuda()
    sa = torch.empty(len(cat), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(["t%d" % i for i in range(a.targets)], [tlen] * a.targets),
                                 keep=(sa, d_seq))
    n_kmers = a.targets * (tlen - a.kmer_len + 1)
    res = dict(tool="hammings_bench", targets=a.targets, target_bp=tlen * a.targets, copies=a.copies, kmer_len=a.kmer_len, rhamm=a.rhamm,
               sensitivity=0, kmers=n_kmers, device=torch.cuda.get_device_name(0), sets=[])
    for both in (False, True):
        h = ix.restricted_hammings(a.kmer_len, a.rhamm, both_strands=both)  # warm-up: sizes the workspace
        wall, dev = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            h = ix.restricted_hammings(a.kmer_len, a.rhamm, both_strands=both)
            wall.append(time.perf_counter() - t0)
            dev.append(ix.hamming_kernel_ms())
        hist = np.bincount(h[h != 0xFF], minlength=a.rhamm + 2)
        res["sets"].append(dict(both_strands=both, kmers_per_s=round(n_kmers / min(wall), 1), wall_ms=[round(1e3 * w, 2) for w in wall],
                                kernel_ms=[round(d, 3) for d in dev], hamming_counts=[int(v) for v in hist]))
    ix.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
