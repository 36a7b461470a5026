"""Time the alignment statistics stage (`k4align -O`, k4_align_stats_dev) through the public binding, with device events after a
warm-up, on 50 M x 100 bp single-end alignments (the C2 shape): reads cut from an iid genome of 24 sequences on either strand with
1 % substitutions, every read accepted.  Two runs: quality bits zero (`-g3`: one band) and random 4-bit scores (four bands).
Beside the times it prints the yardstick: the bytes the stage has to read (read bytes, the 2-bit reference windows, 16-byte hits,
24-byte results, offsets and lengths) over the read rate measured in profiles/d2d_copy.txt.

    python tools/align_stats_bench.py [--reads 50000000] [--genome-mbp 480] [--out profiles/align_stats_bench.json]
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kit4b_amd as k4  # noqa: E402

READ_LEN = 100


def build_index(n_chrom, chrom_len, seed=11):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    n = n_chrom * (chrom_len + 1)
    seq = torch.empty(n, dtype=torch.uint8, device=dev)
    for c in range(n_chrom):
        o = c * (chrom_len + 1)
        seq[o:o + chrom_len] = torch.randint(0, 4, (chrom_len,), dtype=torch.uint8, device=dev, generator=g)
        seq[o + chrom_len] = 7
    sa = torch.empty(n, dtype=torch.int32, device=dev)
    k4.build_sa_device(n, 4, seq.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(n, 4, seq.data_ptr(), sa.data_ptr(), k4.make_entries(["chr%d" % (i + 1) for i in range(n_chrom)], [chrom_len] * n_chrom),
                                 keep=(sa,))
    return ix, seq


def make_batch(seq, n, n_chrom, chrom_len, seed=12):
    """device arrays of n accepted alignments: reads (n * 100 bytes + pad), offs, lens, rr, hits"""
    dev = seq.device
    g = torch.Generator(device=dev).manual_seed(seed)
    chrom = torch.randint(0, n_chrom, (n,), generator=g, device=dev)
    start = torch.randint(0, chrom_len - READ_LEN, (n,), generator=g, device=dev)
    minus = torch.rand(n, generator=g, device=dev) < 0.5
    reads = torch.zeros(n * READ_LEN + 64, dtype=torch.uint8, device=dev)
    ar = torch.arange(READ_LEN, device=dev)
    step = 2_000_000
    for a in range(0, n, step):
        b = min(n, a + step)
        pos = (chrom[a:b] * (chrom_len + 1) + start[a:b])[:, None] + ar[None, :]
        rd = seq[pos]
        m = minus[a:b]
        rd[m] = 3 - rd[m].flip(1)
        sub = torch.rand(rd.shape, generator=g, device=dev) < 0.01
        rd[sub] = (rd[sub] + torch.randint(1, 4, (int(sub.sum()),), generator=g, device=dev, dtype=torch.uint8)) % 4
        reads[a * READ_LEN:b * READ_LEN] = rd.reshape(-1)
        del pos, rd, sub
    offs = torch.arange(n, device=dev, dtype=torch.int64) * READ_LEN
    lens = torch.full((n,), READ_LEN, dtype=torch.int32, device=dev)
    rr = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    rr[:, 0], rr[:, 1], rr[:, 4], rr[:, 5] = 1, 1, 1, 1
    hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    hits[:, 0], hits[:, 1] = (chrom + 1).to(torch.int32), start.to(torch.int32)
    hits[:, 2] = READ_LEN | (torch.where(minus, ord("-"), ord("+")).to(torch.int32) << 16)
    return reads, offs, lens, rr, hits


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


def read_rate():
    """TB/s of a read-only pass, from profiles/d2d_copy.txt"""
    m = re.search(r"read-only sum: ([\d.]+) TB/s", open(os.path.join(ROOT, "profiles", "d2d_copy.txt")).read())
    return float(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--genome-mbp", type=int, default=480)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    k4.lib()
    n_chrom, chrom_len = 24, a.genome_mbp * 1_000_000 // 24
    ix, seq = build_index(n_chrom, chrom_len)
    reads, offs, lens, rr, hits = make_batch(seq, a.reads, n_chrom, chrom_len)
    st = torch.cuda.current_stream().cuda_stream
    n = a.reads
    must_read = n * (READ_LEN + READ_LEN / 4 + 16 + 24 + 8 + 4)
    rate = read_rate()
    rep = dict(reads=n, read_len=READ_LEN, genome_bp=n_chrom * chrom_len, device=torch.cuda.get_device_name(0), reps=a.reps,
               bytes_to_read=must_read, read_rate_TBps=rate, yardstick_ms=must_read / (rate * 1e12) * 1e3)
    for name in ("g3_one_band", "four_bands"):
        if name == "four_bands":
            g = torch.Generator(device="cuda").manual_seed(13)
            reads[:n * READ_LEN] |= torch.randint(0, 16, (n * READ_LEN,), generator=g, device="cuda", dtype=torch.uint8) << 4
        got = []
        stage = lambda: got.append(ix.align_stats(n, 1, READ_LEN, reads, offs, lens, d_rr=rr, d_hits=hits, stream=st))  # noqa: E731
        timed(stage, 2)  # warm-up (code objects, the allocator)
        ms = timed(stage, a.reps)
        s = got[-1]
        assert s["n_accepted"] == n and int(s["q_insts"].sum()) == n * READ_LEN
        rep[name] = dict(stage_ms_median=float(np.median(ms)), stage_ms_min=float(min(ms)), stage_ms_max=float(max(ms)), stage_ms=ms,
                         ratio_to_yardstick=float(np.median(ms)) / rep["yardstick_ms"], bands_live=int((s["q_insts"].sum(axis=1) > 0).sum()),
                         subs=int(s["q_subs"].sum()), uniq_loci=int(s["ent_uniq_loci"].sum()))
        print(name, json.dumps(rep[name]), flush=True)
    ix.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
