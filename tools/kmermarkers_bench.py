"""Times SfxIndex.kmer_cults (CSfxArray::GenKMerCultsCnts, kit4b_amd/csrc/k4_cults.hip) on a GPU: a synthetic pseudo-genome of
--cultivars sequences that descend from one random ancestor by --div substitutions per base, every fourth one reverse complemented;
K-mers of --kmer-len bases found in all cultivars but one, sense only and both strands.  One warm-up, then --repeats sweeps with
room for the whole result in one call (`wall_ms`, `kernel_ms`: the wall clock of the Python call, downloads of the records
included, and the device time of its launches) and as many with SfxIndex.kmer_cults' default room of 2^16 K-mers per call, which
is also the C++ facade's (`default_room_wall_ms`).  Prints one JSON line; --out writes it to a file as well.

When oracle/_ref/ngskit4b is present the index is also written as a .sfx file and the reference's front end (`ngskit4b prekmarkers
-T16 -S0`, kmermarkers.cpp) is timed on it once per strand mode.  Its wall time holds the load of the index, a fixed 10 s wait
for its worker threads (MarkerKMers.cpp:482), its own post-processing and the writing of its file, none of which the device
figures hold: `ref_wall_s` is reported as it is and `ref_sweep_s_at_most`, the wall time less that wait, is an upper bound of its
sweep, not a figure to divide by.  No threshold is set on either.

  python tools/kmermarkers_bench.py --mbp 2 --out profiles/cults_bench.json
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-threads", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import kit4b_amd as k4

    assert torch.cuda.is_available(), "kmermarkers_bench needs a GPU"
    rng = np.random.default_rng(20262)
    tlen = int(a.mbp * 1e6 / a.cultivars)
    anc = rng.integers(0, 4, tlen).astype(np.uint8)
    ts = []
    for c in range(a.cultivars):
        t = anc.copy()
        pos = rng.choice(tlen, size=int(a.div * tlen), replace=False)
        t[pos] = (t[pos] + rng.integers(1, 4, len(pos))) % 4
        ts.append((3 - t[::-1]).copy() if c % 4 == 3 else t)
    cat = np.concatenate([np.concatenate([t, np.array([7], np.uint8)]) for t in ts])
    d_seq = torch.from_numpy(cat).cuda()
    sa = torch.empty(len(cat), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(len(cat), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(["cult%d" % i for i in range(a.cultivars)], [tlen] * a.cultivars),
                                 keep=(sa, d_seq))
    res = dict(tool="kmermarkers_bench", cultivars=a.cultivars, total_bp=tlen * a.cultivars, divergence=a.div, kmer_len=a.kmer_len,
               sfx_elements=len(cat), device=torch.cuda.get_device_name(0), sets=[])
    ref_exe = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")
    with tempfile.TemporaryDirectory() as tmp:
        sfx = os.path.join(tmp, "bench.sfx")
        if os.path.exists(ref_exe):
            ix.write_sfx(sfx)
        for sense_only in (True, False):
            kw = dict(prefix_len=a.kmer_len, min_cultivars=a.cultivars - 1, sense_only=sense_only, max_kmers=1 << 20, max_dist=8 << 20)
            dflt = dict(prefix_len=a.kmer_len, min_cultivars=a.cultivars - 1, sense_only=sense_only)
            r = ix.kmer_cults(**kw)  # warm-up: sizes the workspace
            wall, dev = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                r = ix.kmer_cults(**kw)
                wall.append(time.perf_counter() - t0)
                dev.append(ix.cults_kernel_ms())
            small = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                r2 = ix.kmer_cults(**dflt)
                small.append(time.perf_counter() - t0)
            assert len(r2["kmers"]) == len(r["kmers"]) and r2["n_located"] == r["n_located"]
            s = dict(sense_only=sense_only, located=int(r["n_located"]), reported=len(r["kmers"]), elements_per_s=round(len(cat) / min(wall), 1),
                     wall_ms=[round(1e3 * w, 2) for w in wall], kernel_ms=[round(d, 3) for d in dev],
                     default_room_wall_ms=[round(1e3 * w, 2) for w in small])
            if os.path.exists(ref_exe):
                cmd = [ref_exe, "prekmarkers", "-m%d" % (1 if sense_only else 0), "-k%d" % a.kmer_len, "-s%d" % (a.cultivars - 1), "-S0", "-T%d" % a.ref_threads, "-i", sfx,
                       "-o", os.path.join(tmp, "ref.fa"), "-F", os.path.join(tmp, "ref.log")]
                t0 = time.perf_counter()
                rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
                ref_wall = time.perf_counter() - t0
                s.update(ref_rc=rc, ref_threads=a.ref_threads, ref_wall_s=round(ref_wall, 2), ref_sweep_s_at_most=round(max(ref_wall - 10.0, 0.0), 2))
            res["sets"].append(s)
    ix.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
