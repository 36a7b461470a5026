"""Time the PCR duplicate stage (`k4align -k`, k4_reduce_pcr_dups_dev) with device events after a warm-up, at 50 M reads in two
shapes: C2-like unique loci (random starts over a 3 Gbp genome) and amplicon-like (the reads on 20 000 stacks).  For scale the same
process times a device sort of the same reads' 64-bit coordinate keys (torch.sort), the step the SAM formatter's ordering costs.

    python tools/pcrdup_bench.py [--reads 50000000] [--win 20] [--out profiles/pcrdup_bench.json]
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


def results(n, shape, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = torch.device("cuda")
    rr = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    if shape == "c2":
        chrom = torch.randint(1, 25, (n,), generator=g, device=dev, dtype=torch.int32)
        start = torch.randint(0, 120_000_000, (n,), generator=g, device=dev, dtype=torch.int32)
    else:  # amplicon: 20 000 stacks, each read on one of them
        sites = torch.randint(0, 120_000_000, (20_000,), generator=g, device=dev, dtype=torch.int32)
        sc = torch.randint(1, 25, (20_000,), generator=g, device=dev, dtype=torch.int32)
        pick = torch.randint(0, 20_000, (n,), generator=g, device=dev)
        chrom, start = sc[pick], sites[pick]
    strand = torch.where(torch.rand(n, generator=g, device=dev) < 0.5, ord("+"), ord("-")).to(torch.int32)
    low = torch.randint(0, 4, (n,), generator=g, device=dev, dtype=torch.int32)
    rr[:, 0], rr[:, 1], rr[:, 2], rr[:, 4], rr[:, 5] = 1, 1, low, 1, 1
    hits[:, 0], hits[:, 1] = chrom, start
    hits[:, 2] = 100 | (strand << 16) | (low << 24)
    return rr, hits


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
    ap.add_argument("--win", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    kit4b_amd.lib()
    ix = kit4b_amd.SfxIndex.open(os.path.join(ROOT, "tests", "golden", "g1.sfx"))
    st = torch.cuda.current_stream().cuda_stream
    rep = dict(reads=a.reads, win=a.win, device=torch.cuda.get_device_name(0))
    for shape in ("c2", "amplicon"):
        rr0, hits = results(a.reads, shape)
        rr = rr0.clone()
        n_dups = []

        def stage():
            rr.copy_(rr0)  # (a fresh copy of the results each time: 24 B/read, timed with the stage)
            n_dups.append(ix.reduce_pcr_dups(a.win, a.reads, 1, rr, hits, st))

        timed(stage, 1)  # warm-up (allocations, code objects)
        ms = timed(stage, a.reps)
        copy_ms = timed(lambda: rr.copy_(rr0), a.reps)
        keys = (hits[:, 0].to(torch.int64) << 32) | hits[:, 1].to(torch.int64)
        timed(lambda: torch.sort(keys, stable=True), 1)
        sort_ms = timed(lambda: torch.sort(keys, stable=True), a.reps)
        rep[shape] = dict(stage_ms_median=float(np.median(ms)), stage_ms=ms, copy_ms_median=float(np.median(copy_ms)),
                          sort64_ms_median=float(np.median(sort_ms)), dups=n_dups[-1])
        print(shape, json.dumps(rep[shape]), flush=True)
        del rr0, rr, hits, keys
        torch.cuda.empty_cache()
    ix.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
