"""Time the per-target PE insert length stage (`k4align -3`, k4_pe_insert_dist_dev) through the public binding, with device events
after a warm-up, on 50 M accepted pairs of 100 bp reads made on the device: mates cut from an iid genome 150..700 bases apart with
1 % substitutions, PE1 on either side.  Two shapes: 24 target sequences (a genome: 2 M pairs a target, so the cap of a million pairs
is live) and 100 000 target sequences (a transcriptome: 500 pairs a target).  Beside each the alignment statistics stage
(`-O`, k4_align_stats_dev) is timed on the same records: it is the stage `-3` accompanies.

    python tools/peinserts_bench.py [--pairs 50000000] [--genome-mbp 240] [--out profiles/peinserts_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kit4b_amd as k4  # noqa: E402
from align_stats_bench import READ_LEN, build_index, timed  # noqa: E402


def make_pairs(seq, n_pairs, n_chrom, chrom_len, seed=21):
    """device arrays of n_pairs accepted PE-aligned pairs: pe (2n x 10 int32 = k4_pe_read), reads, offs, lens"""
    dev = seq.device
    g = torch.Generator(device=dev).manual_seed(seed)
    n = 2 * n_pairs
    chrom = torch.randint(0, n_chrom, (n_pairs,), generator=g, device=dev)
    insert = torch.randint(150, min(701, chrom_len), (n_pairs,), generator=g, device=dev)
    left = (torch.rand(n_pairs, generator=g, device=dev, dtype=torch.float64) * (chrom_len - insert)).to(torch.int64)
    first_left = torch.rand(n_pairs, generator=g, device=dev) < 0.5
    start = torch.empty(n, dtype=torch.int64, device=dev)
    start[0::2] = torch.where(first_left, left, left + insert - READ_LEN)
    start[1::2] = torch.where(first_left, left + insert - READ_LEN, left)
    minus = torch.empty(n, dtype=torch.bool, device=dev)
    minus[0::2], minus[1::2] = ~first_left, first_left
    chrom2 = chrom.repeat_interleave(2)
    reads = torch.zeros(n * READ_LEN + 64, dtype=torch.uint8, device=dev)
    ar = torch.arange(READ_LEN, device=dev)
    step = 2_000_000
    for a in range(0, n, step):
        b = min(n, a + step)
        rd = seq[(chrom2[a:b] * (chrom_len + 1) + start[a:b])[:, None] + ar[None, :]]
        m = minus[a:b]
        rd[m] = 3 - rd[m].flip(1)
        sub = torch.rand(rd.shape, generator=g, device=dev) < 0.01
        rd[sub] = (rd[sub] + torch.randint(1, 4, (int(sub.sum()),), generator=g, device=dev, dtype=torch.uint8)) % 4
        reads[a * READ_LEN:b * READ_LEN] = rd.reshape(-1)
        del rd, sub
    offs = torch.arange(n, device=dev, dtype=torch.int64) * READ_LEN
    lens = torch.full((n,), READ_LEN, dtype=torch.int32, device=dev)
    pe = torch.zeros((n, 10), dtype=torch.int32, device=dev)  # nar num_hits inst low_mm pe_aligned rescued | chrom loci len/strand/mm ext
    pe[:, 0], pe[:, 1], pe[:, 2], pe[:, 4] = 1, 1, 1, 1
    pe[:, 6], pe[:, 7] = (chrom2 + 1).to(torch.int32), start.to(torch.int32)
    pe[:, 8] = READ_LEN | (torch.where(minus, ord("-"), ord("+")).to(torch.int32) << 16)
    return pe, reads, offs, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--genome-mbp", type=int, default=240)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    k4.lib()
    st = torch.cuda.current_stream().cuda_stream
    rep = dict(pairs=a.pairs, read_len=READ_LEN, device=torch.cuda.get_device_name(0), reps=a.reps)
    for name, n_chrom in (("targets_24", 24), ("targets_100000", 100_000)):
        chrom_len = a.genome_mbp * 1_000_000 // n_chrom
        ix, seq = build_index(n_chrom, chrom_len)
        pe, reads, offs, lens = make_pairs(seq, a.pairs, n_chrom, chrom_len)
        got, yard = [], []
        stage = lambda: got.append(ix.pe_insert_dist(a.pairs, pe, stream=st))  # noqa: E731
        stats = lambda: yard.append(ix.align_stats(2 * a.pairs, 1, READ_LEN, reads, offs, lens, d_pe=pe, stream=st))  # noqa: E731
        timed(stage, 2)  # warm-up (code objects, the allocator)
        ms = timed(stage, a.reps)
        timed(stats, 1)
        ms_stats = timed(stats, a.reps)
        d = got[-1]
        want = min(a.pairs // n_chrom, 1_000_000)
        assert len(d["entry_id"]) == n_chrom and int(d["dist"].sum()) == int(d["tot_pes"].sum()) and yard[-1]["n_accepted"] == 2 * a.pairs
        assert int(d["tot_pes"].sum()) == a.pairs if a.pairs // n_chrom < 900_000 else (d["tot_pes"] <= 1_000_000).all()
        rep[name] = dict(n_targets=n_chrom, genome_bp=n_chrom * chrom_len, pairs_counted=int(d["tot_pes"].sum()), pairs_per_target=want,
                         median_of_medians=int(np.median(d["median"])), stage_ms_median=float(np.median(ms)), stage_ms_min=float(min(ms)),
                         stage_ms_max=float(max(ms)), stage_ms=ms, align_stats_ms_median=float(np.median(ms_stats)), align_stats_ms=ms_stats,
                         ratio_to_align_stats=float(np.median(ms)) / float(np.median(ms_stats)))
        print(name, json.dumps(rep[name]), flush=True)
        ix.close()
        del pe, reads, offs, lens, seq
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
