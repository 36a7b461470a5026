"""Time the start-site octamer stage (`k4align -8`, k4_site_prefs_dev) with device events after a warm-up, at 50 M accepted 100 bp
reads on a device-built genome, in two shapes -- uniform starts, and skewed (half of the reads on 1000 sites) -- and for both forms of
its histogram step (K4_SITEPREFS_HIST=atomic: global atomics with wave-level pre-aggregation; sort: key sort + run lengths).

The yardstick is the bytes the stage must read -- result (24 B), hit record (16 B) and two packed reference words (8 B) per read --
over the read rate in profiles/d2d_copy.txt.

    python tools/siteprefs_bench.py [--reads 50000000] [--out profiles/siteprefs_bench.json]
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

N_SEQ, SEQ_LEN = 24, 1_000_000


def genome_index():
    g = torch.Generator(device="cuda").manual_seed(11)
    seq = torch.randint(0, 4, (N_SEQ, SEQ_LEN + 1), generator=g, device="cuda", dtype=torch.uint8)
    seq[:, SEQ_LEN] = 7  # one EOS behind every sequence
    seq = seq.reshape(-1).contiguous()
    sa = torch.empty(seq.numel(), dtype=torch.int32, device="cuda")
    k4.build_sa_device(seq.numel(), 4, seq.data_ptr(), sa.data_ptr())
    return k4.SfxIndex.from_device(seq.numel(), 4, seq.data_ptr(), sa.data_ptr(), k4.make_entries(["s%02d" % i for i in range(N_SEQ)], [SEQ_LEN] * N_SEQ),
                                   keep=(sa, seq))


def results(n, shape, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = torch.device("cuda")
    rr = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    chrom = torch.randint(1, N_SEQ + 1, (n,), generator=g, device=dev, dtype=torch.int32)
    start = torch.randint(0, SEQ_LEN - 100, (n,), generator=g, device=dev, dtype=torch.int32)
    strand = torch.where(torch.rand(n, generator=g, device=dev) < 0.5, ord("+"), ord("-")).to(torch.int32)
    if shape == "skewed":  # half of the reads on 1000 sites
        sc = torch.randint(1, N_SEQ + 1, (1000,), generator=g, device=dev, dtype=torch.int32)
        ss = torch.randint(0, SEQ_LEN - 100, (1000,), generator=g, device=dev, dtype=torch.int32)
        sd = torch.where(torch.rand(1000, generator=g, device=dev) < 0.5, ord("+"), ord("-")).to(torch.int32)
        pick = torch.randint(0, 1000, (n,), generator=g, device=dev)
        hot = torch.rand(n, generator=g, device=dev) < 0.5
        chrom, start, strand = torch.where(hot, sc[pick], chrom), torch.where(hot, ss[pick], start), torch.where(hot, sd[pick], strand)
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    k4.lib()
    ix = genome_index()
    st = torch.cuda.current_stream().cuda_stream
    rate = float(re.search(r"read-only sum: ([\d.]+) TB/s", open(os.path.join(ROOT, "profiles", "d2d_copy.txt")).read()).group(1))
    need = a.reads * (24 + 16 + 8)
    rep = dict(reads=a.reads, read_len=100, genome_bp=N_SEQ * SEQ_LEN, device=torch.cuda.get_device_name(0), reps=a.reps, bytes_to_read=need,
               read_rate_TBps=rate, yardstick_ms=need / (rate * 1e12) * 1e3)
    for shape in ("uniform", "skewed"):
        rr, hits = results(a.reads, shape)
        rep[shape] = {}
        tabs = {}
        for form in ("atomic", "sort"):
            os.environ["K4_SITEPREFS_HIST"] = form
            got = []
            stage = lambda: got.append(ix.site_prefs(a.reads, 1, -4, d_rr=rr, d_hits=hits, stream=st))  # noqa: E731
            timed(stage, 1)  # warm-up (allocations, code objects)
            ms = timed(stage, a.reps)
            tabs[form] = got[-1]
            rep[shape][form] = dict(stage_ms_median=float(np.median(ms)), stage_ms_min=min(ms), stage_ms_max=max(ms), stage_ms=ms,
                                    ratio_to_yardstick=float(np.median(ms)) / rep["yardstick_ms"], counted=got[-1]["n_counted"],
                                    sites=int(got[-1]["num_sites"].sum()), max_occs=int(got[-1]["num_occs"].max()))
            print(shape, form, json.dumps(rep[shape][form]), flush=True)
        assert all(np.array_equal(tabs["atomic"][k], tabs["sort"][k]) for k in ("num_occs", "num_sites"))
        del rr, hits
        torch.cuda.empty_cache()
    os.environ.pop("K4_SITEPREFS_HIST", None)
    ix.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
