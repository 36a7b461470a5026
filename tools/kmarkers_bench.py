"""Times SfxIndex.species_kmers (`ngskit4b kmarkers`, kit4b_amd/csrc/k4_kmarkers.hip) on a GPU: a synthetic pseudo-genome of
--cultivars sequences that descend from one random ancestor by --div substitutions per base; cultivar 0 is the target.  One warm-up,
then --repeats scans: `kernel_ms` is the device time of a call's launches, `wall_ms` the wall clock of the Python call with the
download of the status bytes, `ns_per_position` and `positions_per_s` come from the best kernel time over the target's start loci.
Prints one JSON line; --out writes it to a file as well.

When oracle/_ref/ngskit4b is present the index is also written as a .sfx file and the reference's front end (`ngskit4b kmarkers
-T16`) is timed on it once.  Its wall time holds the load of the index and a fixed 10 s wait for its worker threads
(LocKMers.cpp:806-811), which the device figures do not hold: `ref_wall_s` is reported as it is and `ref_scan_s_at_most`, the wall
time less that wait, is an upper bound of its scan, not a figure to divide by.  The front end hands -s to the scan as the Hamming
separation (see kit4b_amd.kmarkers_fasta), so it is run in mode 2 with -s<min-hamming>.  No threshold is set on either.

  python tools/kmarkers_bench.py --mbp 2 --out profiles/kmarkers_bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=2.0, help="total length of all cultivars")
    ap.add_argument("--cultivars", type=int, default=5)
    ap.add_argument("--div", type=float, default=0.01)
    ap.add_argument("--kmer-len", type=int, default=50)
    ap.add_argument("--min-hamming", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-threads", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import kit4b_amd as k4

    assert torch.cuda.is_available(), "kmarkers_bench needs a GPU"
    rng = np.random.default_rng(20273)
    tlen = int(a.mbp * 1e6 / a.cultivars)
    anc = rng.integers(0, 4, tlen).astype(np.uint8)
    ts = []
    for c in range(a.cultivars):
        t = anc.copy()
        pos = rng.choice(tlen, size=int(a.div * tlen), replace=False)
        t[pos] = (t[pos] + rng.integers(1, 4, len(pos))) % 4
        ts.append(t)
    cat = np.concatenate([np.concatenate([t, np.array([7], np.uint8)]) for t in ts])
    d_seq = torch.from_numpy(cat).cuda()
    sa = torch.empty(len(cat), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr())
    names = ["cult%d" % i for i in range(a.cultivars)]
    ix = k4.SfxIndex.from_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(names, [tlen] * a.cultivars), keep=(sa, d_seq))
    res = dict(tool="kmarkers_bench", cultivars=a.cultivars, total_bp=tlen * a.cultivars, positions=tlen, divergence=a.div, kmer_len=a.kmer_len,
               min_hamming=a.min_hamming, device=torch.cuda.get_device_name(0))
    kw = dict(kmer_len=a.kmer_len, min_hamming=a.min_hamming, mode=2, prefix_len=a.kmer_len // 2, min_with_prefix=1)
    status, tallies = ix.species_kmers([1], **kw)  # warm-up: sizes the workspace
    wall, dev = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        status, tallies = ix.species_kmers([1], **kw)
        wall.append(time.perf_counter() - t0)
        dev.append(ix.kmarkers_kernel_ms())
    res.update(tallies=tallies, status_counts=np.bincount(status, minlength=8).tolist(), wall_ms=[round(1e3 * w, 2) for w in wall],
               kernel_ms=[round(d, 3) for d in dev], ns_per_position=round(1e6 * min(dev) / tlen, 2), positions_per_s=round(tlen / (1e-3 * min(dev)), 1))
    ref_exe = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")
    if os.path.exists(ref_exe):
        with tempfile.TemporaryDirectory() as tmp:
            sfx = os.path.join(tmp, "bench.sfx")
            ix.write_sfx(sfx)
            cmd = [ref_exe, "kmarkers", "-m2", "-k%d" % a.kmer_len, "-p%d" % (a.kmer_len // 2), "-s%d" % a.min_hamming, "-K1", "-c", "bench", "-C", names[0],
                   "-T%d" % a.ref_threads, "-i", sfx, "-o", os.path.join(tmp, "ref.fa"), "-F", os.path.join(tmp, "ref.log")]
            t0 = time.perf_counter()
            rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
            ref_wall = time.perf_counter() - t0
            n_ref = open(os.path.join(tmp, "ref.fa"), "rb").read().count(b">") if rc == 0 else -1
            res.update(ref_rc=rc, ref_threads=a.ref_threads, ref_wall_s=round(ref_wall, 2), ref_scan_s_at_most=round(max(ref_wall - 10.0, 0.0), 2),
                       ref_markers=n_ref)
    ix.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
