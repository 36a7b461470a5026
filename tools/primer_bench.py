"""Time the 5' PCR primer correction stage (`k4align -6`, k4_pcr5_primer_correct_dev) with device events after a warm-up: 50 M accepted
100 bp records over g1, 2 % of them over the rate (so that they reach the stage's second phase: target fetch, walks, byte stores).
For scale the same process times k4_filter_chroms_dev on the same records -- the other stage that is one streaming pass over the
result records.  Records and reads are restored from a copy before every run, outside of the timed span.

    python tools/primer_bench.py [--reads 50000000] [--subs 1] [--out profiles/primer_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kit4b_amd  # noqa: E402

READ_LEN = 100
CHROM_LENS = [60000, 40000, 25000]  # the long sequences of tests/golden/g1.sfx


def records(n, subs, over_share, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = torch.device("cuda")
    rr = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    chrom = torch.randint(0, 3, (n,), generator=g, device=dev)
    clen = torch.tensor(CHROM_LENS, device=dev)[chrom]
    start = (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * (clen - READ_LEN + 1)).to(torch.int32)
    strand = torch.where(torch.rand(n, generator=g, device=dev) < 0.5, ord("+"), ord("-")).to(torch.int32)
    max_mms = (subs * READ_LEN + 50) // 100
    over = torch.rand(n, generator=g, device=dev) < over_share
    low = torch.where(over, max_mms + torch.randint(1, 4, (n,), generator=g, device=dev), torch.randint(0, max_mms + 1, (n,), generator=g, device=dev)).to(torch.int32)
    rr[:, 0], rr[:, 1], rr[:, 2], rr[:, 4], rr[:, 5] = 1, 1, low, 1, 1
    hits[:, 0], hits[:, 1] = (chrom + 1).to(torch.int32), start
    hits[:, 2] = READ_LEN | (strand << 16) | (low << 24)
    reads = torch.randint(0, 4, (n * READ_LEN + 64,), generator=g, device=dev, dtype=torch.uint8)  # (random bases: most of the 12 differ)
    offs = torch.arange(n, device=dev, dtype=torch.int64) * READ_LEN
    lens = torch.full((n,), READ_LEN, dtype=torch.int32, device=dev)
    return rr, hits, reads, offs, lens, int(over.sum())


def timed(fn, reps, before=None):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps):
        if before:
            before()
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
    ap.add_argument("--subs", type=int, default=1)
    ap.add_argument("--over", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    kit4b_amd.lib()
    ix = kit4b_amd.SfxIndex.open(os.path.join(ROOT, "tests", "golden", "g1.sfx"))
    st = torch.cuda.current_stream().cuda_stream
    rr0, hits0, reads0, offs, lens, n_over = records(a.reads, a.subs, a.over)
    rr, hits, reads = rr0.clone(), hits0.clone(), reads0.clone()
    totals = []

    def restore():
        rr.copy_(rr0), hits.copy_(hits0), reads.copy_(reads0)

    def stage():
        totals.append(ix.pcr5_primer_correct(a.subs, a.reads, 1, reads, offs, lens, d_rr=rr, d_hits=hits, stream=st))

    timed(stage, 1, restore)  # warm-up (allocations, code objects)
    ms = timed(stage, a.reps, restore)
    accept = torch.ones(8, dtype=torch.uint8, device="cuda")
    chroms = lambda: ix.filter_chroms(accept, a.reads, 1, d_rr=rr, d_hits=hits, stream=st)  # noqa: E731
    timed(chroms, 1, restore)
    chrom_ms = timed(chroms, a.reps, restore)
    rep = dict(reads=a.reads, read_len=READ_LEN, max_subs=a.subs, over_the_rate=n_over, device=torch.cuda.get_device_name(0),
               stage_ms_median=float(np.median(ms)), stage_ms=ms, totals=list(totals[-1]),
               filter_chroms_ms_median=float(np.median(chrom_ms)), filter_chroms_ms=chrom_ms,
               record_bytes_per_read=24 + 16 + 4)
    ix.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
