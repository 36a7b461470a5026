"""Time `kalign -B` on the device (k4_priority.hip): 100 bp reads drawn from a synthetic 24-sequence genome built on the device, aligned
(i) with no table set, (ii) with a table over ~1 % of the genome, (iii) over ~50 %; then the filter stage on the results.  With a table
the call is split by the library itself (k4_priority_times: host clock around stream waits, kernel timing on) into the wide pass
(max_ml + 10 hits), the select kernel with the listing of the reads that need the normal call, and the normal pass with the scatter.

    python tools/priority_bench.py [--reads 20000000] [--seq-mbp 4] [--out profiles/priority_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kit4b_amd as k4  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--seq-mbp", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    k4.lib()
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(11)
    n_chrom, L, rl, n = 24, int(a.seq_mbp * 1e6), 100, a.reads
    seq = torch.randint(0, 4, (n_chrom * (L + 1),), generator=g, device=dev, dtype=torch.uint8)
    seq[L::L + 1] = 7
    sa = torch.empty(len(seq), dtype=torch.int32, device=dev)
    k4.build_sa_device(len(seq), 4, seq.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(len(seq), 4, seq.data_ptr(), sa.data_ptr(), k4.make_entries(["chr%d" % (i + 1) for i in range(n_chrom)], [L] * n_chrom),
                                 keep=(sa, seq))
    ix.set_max_iter(5000)
    st = torch.cuda.current_stream().cuda_stream
    # reads: exact copies of the '+' strand (every one is unique in a random genome)
    chrom = torch.randint(0, n_chrom, (n,), generator=g, device=dev, dtype=torch.int64)
    start = torch.randint(0, L - rl, (n,), generator=g, device=dev, dtype=torch.int64)
    pos = chrom * (L + 1) + start
    reads = torch.empty(n * rl + 64, dtype=torch.uint8, device=dev)
    step = 2_000_000
    for s in range(0, n, step):
        p = pos[s:s + step]
        reads[s * rl:(s + len(p)) * rl] = seq[(p[:, None] + torch.arange(rl, device=dev)[None, :]).reshape(-1)]
    offs = torch.arange(n, device=dev, dtype=torch.int64) * rl
    lens = torch.full((n,), rl, device=dev, dtype=torch.int32)
    rr = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    kp = k4.KalignParams(2, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0)
    ix.reserve(n, rl, 11)
    ix.enable_kernel_timing(True)
    rep = dict(reads=n, read_len=rl, genome_bp=n_chrom * L, device=torch.cuda.get_device_name(0), max_subs=2, max_ml=1)

    def run(name, cover):
        if cover:
            span = 2000
            per = max(1, int(cover * L / span))
            s = (np.arange(per, dtype=np.int64) * (L // per)).astype(np.uint32)
            ids = np.repeat(np.arange(1, n_chrom + 1, dtype=np.uint32), per)
            ix.set_priority_regions(ids, np.tile(s, n_chrom), np.tile(s + span - 1, n_chrom))
        else:
            ix.set_priority_regions()
        rows = []
        for k in range(a.reps + 1):
            torch.cuda.synchronize()
            ix.kernel_times_split()
            ix.priority_times()
            t0 = time.perf_counter()
            ix.kalign_batch_dev(kp, n, rl, reads.data_ptr(), offs.data_ptr(), lens.data_ptr(), rr.data_ptr(), hits.data_ptr(), st)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            step_ms, gen_ms, _ = ix.kernel_times_split()
            ms, rd = ix.priority_times()
            if k:  # (the first run is the warm-up)
                rows.append(dict(wall_ms=wall, align_kernels_ms=step_ms + gen_ms, wide_pass_ms=ms[0], select_ms=ms[1], normal_pass_ms=ms[2],
                                 reads_normal_pass=rd[1]))
        acc = int((rr[:, 4] == 1).sum())
        out = dict(runs=rows, wall_ms_median=float(np.median([r["wall_ms"] for r in rows])), accepted=acc)
        if cover:
            t0 = time.perf_counter()
            out["filter_marked"] = ix.filter_priority_regions(n, 1, d_rr=rr, d_hits=hits, stream=st)
            out["filter_ms"] = (time.perf_counter() - t0) * 1e3
        rep[name] = out
        print(name, json.dumps(out), flush=True)

    run("no_table", 0)
    run("table_1pct", 0.01)
    run("table_50pct", 0.5)
    run("no_table_again", 0)
    ix.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rep, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
