"""Time the packed-base-allele stage (`k4align -M3`, k4_pba_run_dev) on synthetic alignments over a device-built genome of long
sequences, at about 1x and about 30x coverage, after a warm-up: the whole stage, and per chromosome its memset, pile-up,
classification + coverage pass, downloads and host WIG walk (the stage's own K4_PBA_TIMES trace).  The SNP stage (k4_snp_run_dev),
which shares the pile-up, runs on the same alignments for comparison.

The yardstick of the classification pass is the bytes it must move -- seven 4-byte counts read, one PBA byte and one coverage byte
written per locus -- over the streaming rates in profiles/d2d_copy.txt.

    python tools/pba_bench.py [--seqs 2] [--seq-len 250000000] [--out profiles/pba_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kit4b_amd as k4  # noqa: E402

READ_LEN = 100


def genome_index(n_seq, seq_len):
    g = torch.Generator(device="cuda").manual_seed(13)
    seq = torch.randint(0, 4, (n_seq, seq_len + 1), generator=g, device="cuda", dtype=torch.uint8)
    seq[:, seq_len] = 7  # one EOS behind every sequence
    seq = seq.reshape(-1).contiguous()
    sa = torch.empty(seq.numel(), dtype=torch.int32, device="cuda")
    k4.build_sa_device(seq.numel(), 4, seq.data_ptr(), sa.data_ptr())
    return k4.SfxIndex.from_device(seq.numel(), 4, seq.data_ptr(), sa.data_ptr(), k4.make_entries(["s%02d" % i for i in range(n_seq)], [seq_len] * n_seq),
                                   keep=(sa, seq))


def alignments(n, n_seq, seq_len, seed):
    """n accepted 100 bp alignments with uniform starts and random read bases (the pile-up's work does not depend on what it counts)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = torch.device("cuda")
    rr = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    rr[:, 0], rr[:, 1], rr[:, 4], rr[:, 5] = 1, 1, 1, 1
    hits[:, 0] = torch.randint(1, n_seq + 1, (n,), generator=g, device=dev, dtype=torch.int32)
    hits[:, 1] = torch.randint(0, seq_len - READ_LEN, (n,), generator=g, device=dev, dtype=torch.int32)
    strand = torch.where(torch.rand(n, generator=g, device=dev) < 0.5, ord("+"), ord("-")).to(torch.int32)
    hits[:, 2] = READ_LEN | (strand << 16)
    reads = torch.randint(0, 4, (n * READ_LEN + 16,), generator=g, device=dev, dtype=torch.uint8)
    offs = torch.arange(n, device=dev, dtype=torch.int64) * READ_LEN
    lens = torch.full((n,), READ_LEN, dtype=torch.int32, device=dev)
    return rr, hits, reads, offs, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=2)
    ap.add_argument("--seq-len", type=int, default=250_000_000)
    ap.add_argument("--coverage", type=float, nargs="+", default=[1.0, 30.0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = k4.lib()
    ix = genome_index(a.seqs, a.seq_len)
    txt = open(os.path.join(ROOT, "profiles", "d2d_copy.txt")).read()
    copy_rate = float(re.search(r"copy \(read\+write\): ([\d.]+) TB/s", txt).group(1))
    read_rate = float(re.search(r"read-only sum: ([\d.]+) TB/s", txt).group(1))
    per_locus = 7 * 4 + 2
    rep = dict(seqs=a.seqs, seq_len=a.seq_len, read_len=READ_LEN, device=torch.cuda.get_device_name(0), reps=a.reps, classify_bytes_per_locus=per_locus,
               copy_rate_TBps=copy_rate, read_rate_TBps=read_rate, classify_yardstick_ms_per_chrom=a.seq_len * per_locus / (read_rate * 1e12) * 1e3,
               runs={})

    class SnpFiles(C.Structure):
        _fields_ = [("snp", C.c_void_p), ("snp_bytes", C.c_uint64), ("n_snps", C.c_uint64), ("wig", C.c_void_p), ("wig_bytes", C.c_uint64),
                    ("disnp", C.c_void_p), ("disnp_bytes", C.c_uint64), ("trisnp", C.c_void_p), ("trisnp_bytes", C.c_uint64)]

    for cov in a.coverage:
        n = int(cov * a.seqs * a.seq_len / READ_LEN)
        rr, hits, reads, offs, lens = alignments(n, a.seqs, a.seq_len, 7)
        head = (ix.h, 0, n, rr.data_ptr(), hits.data_ptr(), 1, None, reads.data_ptr(), offs.data_ptr(), lens.data_ptr())

        def pba():
            f = k4.PbaFiles()
            ix._ck(L.k4_pba_run_dev(*head, b"bench", b"bench", C.byref(f), 0))
            sizes = (f.pba_bytes, f.wig_bytes, f.n_chroms)
            L.k4_free_host(f.pba)
            L.k4_free_host(f.wig)
            return sizes

        def snp():
            f = SnpFiles()
            ix._ck(L.k4_snp_run_dev(ix.h, 0, *head[1:], 5, 0.05, 25.0, C.byref(f), 0))
            for k in ("snp", "wig", "disnp", "trisnp"):
                L.k4_free_host(getattr(f, k))
            return f.wig_bytes

        run = {}
        for name, fn in (("pba", pba), ("snp", snp)):
            fn()  # warm-up (allocations, code objects)
            secs = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                secs.append(time.perf_counter() - t0)
            run[name] = dict(stage_s_median=float(np.median(secs)), stage_s=secs, out=out)
        with tempfile.TemporaryDirectory() as tmp:  # one more PBA run with the stage's own per-chromosome trace
            os.environ["K4_PBA_TIMES"] = os.path.join(tmp, "times.txt")
            pba()
            os.environ.pop("K4_PBA_TIMES")
            lines = open(os.path.join(tmp, "times.txt")).read().splitlines()
        chroms, walks = [], []
        for ln in lines:
            f = ln.split()
            if f[0] == "walk":
                walks.append(float(f[2]))
            else:
                d = dict(zip(f[2::2], f[3::2]))
                chroms.append({k: (float(v) if k.endswith("_ms") else int(v)) for k, v in d.items()})
        run["per_chrom"] = chroms
        run["wig_walk_ms"] = walks
        cls = float(np.median([c["classify_ms"] for c in chroms]))
        run["classify_ms_median"] = cls
        run["classify_TBps"] = a.seq_len * per_locus / (cls * 1e-3) / 1e12
        run["classify_fraction_of_read_rate"] = run["classify_TBps"] / read_rate
        run["pba_over_snp"] = run["pba"]["stage_s_median"] / run["snp"]["stage_s_median"]
        rep["runs"]["%gx" % cov] = dict(reads=n, **run)
        print("%gx" % cov, json.dumps(rep["runs"]["%gx" % cov]), flush=True)
        del rr, hits, reads, offs, lens
        torch.cuda.empty_cache()
    ix.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
