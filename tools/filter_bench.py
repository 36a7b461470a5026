"""Time the two filter stages (k4_filter_chroms_dev, k4_filter_loci_constraints_dev; `k4align --chromexclude / -5`) with device events
after a warm-up, at 50 M accepted 100 bp reads spread over a synthetic 24-sequence genome built on the device: (i) the chromosome
mask alone, (ii) 6400 `R` constraints covering ~1 % of the genome, (iii) 6400 covering ~50 %.  The yardstick is the time the bytes a
stage must read take at the device's measured read bandwidth (profiles/d2d_copy.txt): rr + hit records once, plus the bases of the
reads that overlap a constraint.

    python tools/filter_bench.py [--reads 50000000] [--seq-mbp 4] [--out profiles/filter_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kit4b_amd as k4  # noqa: E402

READ_TBS = 5.92  # read-only sum, profiles/d2d_copy.txt


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--seq-mbp", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
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
    st = torch.cuda.current_stream().cuda_stream
    chrom = torch.randint(1, n_chrom + 1, (n,), generator=g, device=dev, dtype=torch.int32)
    start = torch.randint(0, L - rl, (n,), generator=g, device=dev, dtype=torch.int32)
    strand = torch.where(torch.rand(n, generator=g, device=dev) < 0.5, ord("+"), ord("-")).to(torch.int32)
    rr0 = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    rr0[:, 0], rr0[:, 1], rr0[:, 4], rr0[:, 5] = 1, 1, 1, 1
    hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    hits[:, 0], hits[:, 1], hits[:, 2] = chrom, start, rl | (strand << 16)
    reads = torch.randint(0, 4, (n * rl + 64,), generator=g, device=dev, dtype=torch.uint8)
    offs = torch.arange(n, device=dev, dtype=torch.int64) * rl
    lens = torch.full((n,), rl, device=dev, dtype=torch.int32)
    rr = rr0.clone()
    rep = dict(reads=n, read_len=rl, genome_bp=n_chrom * L, device=torch.cuda.get_device_name(0), read_tb_s=READ_TBS)
    copy_ms = float(np.median(timed(lambda: rr.copy_(rr0), a.reps)))
    rep["rr_restore_copy_ms"] = copy_ms

    def report(name, fn, bytes_read, extra):
        marked = []

        def stage():
            rr.copy_(rr0)  # (a fresh copy of the results each time, timed with the stage and taken off below)
            marked.append(fn())

        timed(stage, 1)  # warm-up
        ms = timed(stage, a.reps)
        yard = bytes_read / (READ_TBS * 1e12) * 1e3
        med = float(np.median(ms)) - copy_ms
        rep[name] = dict(stage_ms_median=med, stage_ms_with_restore=ms, marked=marked[-1], yardstick_bytes=bytes_read, yardstick_ms=yard,
                         times_yardstick=med / yard, **extra)
        print(name, json.dumps(rep[name]), flush=True)

    mask = np.ones(n_chrom + 1, np.uint8)
    mask[[3, 7, 23]] = 0
    d_mask = torch.from_numpy(mask).to(dev)
    report("chrom_mask", lambda: ix.filter_chroms(d_mask, n, 1, d_rr=rr, d_hits=hits, stream=st), n * 40, {})
    rng = np.random.default_rng(5)
    for name, cover in (("loci_1pct", 0.01), ("loci_50pct", 0.5)):
        span = max(1, int(cover * n_chrom * L / 6400))
        t = np.zeros(6400, k4.LOCI_CONSTRAINT_DTYPE)
        t["chrom_id"] = np.arange(6400) % n_chrom + 1
        per = 6400 // n_chrom + 1
        slot = (np.arange(6400) // n_chrom) * (L // per)  # evenly spread, not overlapping
        t["start"] = slot + rng.integers(0, max(1, L // per - span), 6400)
        t["end"] = np.minimum(t["start"] + span - 1, L - 1)
        t["bits"] = 16
        s64, c64 = start.to(torch.int64), chrom.to(torch.int64)
        ov = torch.zeros(n, dtype=torch.bool, device=dev)
        for c in range(1, n_chrom + 1):  # which reads overlap a constraint (for the yardstick's byte count)
            tc = t[t["chrom_id"] == c]
            order = np.argsort(tc["start"])
            ts = torch.from_numpy(tc["start"][order].astype(np.int64)).to(dev)
            te = torch.from_numpy(tc["end"][order].astype(np.int64)).to(dev)
            sel = torch.nonzero(c64 == c).squeeze(1)
            k = torch.searchsorted(ts, s64[sel] + rl - 1, right=True) - 1  # the last constraint starting at or before the read's end
            ov[sel] = (k >= 0) & (te[k.clamp(min=0)] >= s64[sel])
        n_ov = int(ov.sum())
        report(name, lambda: ix.filter_loci_constraints(t, n, 1, reads, offs, lens, d_rr=rr, d_hits=hits, stream=st), n * 40 + n_ov * (rl + 12),
               dict(constraint_span=span, reads_overlapping=n_ov))
    ix.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
