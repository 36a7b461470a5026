"""Time a SNP run (k4_snp_run_dev / k4_snp_run2_dev) in three forms on the same device-resident alignments: plain, with the SNP
centroids (-7), and with marker sequences (-K).  The genome is built on the device; the reads are drawn from a copy of it with a
substitution every ~1000 bases, plus sequencing errors, so that the run has real candidates: the marker kernel has work and the
centroid table fills.  After a warm-up, `--reps` runs of each form; the median and every sample are reported.

A library without k4_snp_run2_dev (an earlier commit) runs the plain form only: that is how the plain run is compared across commits.

    python tools/markers_bench.py [--seqs 2] [--seq-len 50000000] [--coverage 10] [--marker-len 100] [--out profiles/markers_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kit4b_amd as k4  # noqa: E402

READ_LEN = 100


class SnpFiles(C.Structure):
    _fields_ = [("snp", C.c_void_p), ("snp_bytes", C.c_uint64), ("n_snps", C.c_uint64), ("wig", C.c_void_p), ("wig_bytes", C.c_uint64),
                ("disnp", C.c_void_p), ("disnp_bytes", C.c_uint64), ("trisnp", C.c_void_p), ("trisnp_bytes", C.c_uint64)]


def genome(n_seq, seq_len):
    g = torch.Generator(device="cuda").manual_seed(13)
    seq = torch.randint(0, 4, (n_seq, seq_len + 1), generator=g, device="cuda", dtype=torch.uint8)
    seq[:, seq_len] = 7  # one EOS behind every sequence
    return seq


def alignments(seq, n, seed):
    """n accepted '+' strand alignments of READ_LEN bases, read from a copy of the genome with a substitution every ~1000 bases and
    an error every ~200 read bases"""
    n_seq, seq_len = seq.shape[0], seq.shape[1] - 1
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = torch.device("cuda")
    mut = seq.clone()
    at = torch.rand(mut.shape, generator=g, device=dev) < 1e-3
    at[:, seq_len] = False
    mut[at] = (mut[at] + torch.randint(1, 4, (int(at.sum()),), generator=g, device=dev, dtype=torch.uint8)) % 4
    rr = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    rr[:, 0], rr[:, 1], rr[:, 4], rr[:, 5] = 1, 1, 1, 1
    chrom = torch.randint(0, n_seq, (n,), generator=g, device=dev, dtype=torch.int64)
    start = torch.randint(0, seq_len - READ_LEN, (n,), generator=g, device=dev, dtype=torch.int64)
    hits[:, 0] = (chrom + 1).to(torch.int32)
    hits[:, 1] = start.to(torch.int32)
    hits[:, 2] = READ_LEN | (ord("+") << 16)
    reads = torch.empty(n * READ_LEN + 16, dtype=torch.uint8, device=dev)
    flat, step = mut.reshape(-1), 1 << 20
    for a in range(0, n, step):  # (gathered in pieces: the index tensor of a piece stays below 1 GB)
        b = min(n, a + step)
        idx = (chrom[a:b] * (seq_len + 1) + start[a:b])[:, None] + torch.arange(READ_LEN, device=dev)[None, :]
        piece = flat[idx]
        err = torch.rand(piece.shape, generator=g, device=dev) < 5e-3
        piece[err] = (piece[err] + 1) % 4
        reads[a * READ_LEN:b * READ_LEN] = piece.reshape(-1)
    reads[n * READ_LEN:] = 0
    offs = torch.arange(n, device=dev, dtype=torch.int64) * READ_LEN
    lens = torch.full((n,), READ_LEN, dtype=torch.int32, device=dev)
    return rr, hits, reads, offs, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=2)
    ap.add_argument("--seq-len", type=int, default=50_000_000)
    ap.add_argument("--coverage", type=float, default=10.0)
    ap.add_argument("--marker-len", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = k4.lib()
    seq = genome(a.seqs, a.seq_len)
    flat = seq.reshape(-1).contiguous()
    sa = torch.empty(flat.numel(), dtype=torch.int32, device="cuda")
    k4.build_sa_device(flat.numel(), 4, flat.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(flat.numel(), 4, flat.data_ptr(), sa.data_ptr(), k4.make_entries(["s%02d" % i for i in range(a.seqs)], [a.seq_len] * a.seqs),
                                 keep=(sa, flat))
    n = int(a.coverage * a.seqs * a.seq_len / READ_LEN)
    rr, hits, reads, offs, lens = alignments(seq, n, 7)
    head = (ix.h, 0, 0, n, rr.data_ptr(), hits.data_ptr(), 1, None, reads.data_ptr(), offs.data_ptr(), lens.data_ptr(), 5, 0.05, 25.0)
    has2 = hasattr(k4, "SnpFiles2")

    def plain():
        f = SnpFiles()
        ix._ck(L.k4_snp_run_dev(*head, C.byref(f), 0))
        for k in ("snp", "wig", "disnp", "trisnp"):
            L.k4_free_host(getattr(f, k))
        return dict(n_snps=f.n_snps, snp_bytes=f.snp_bytes)

    def run2(marker_len, centroids):
        def fn():
            f = k4.SnpFiles2()
            o = k4.SnpOpts(marker_len, 1 if centroids else 0, k4.DFLT_MARKER_POLY_THRES)
            ix._ck(L.k4_snp_run2_dev(*head, C.byref(o), C.byref(f), 0))
            for k in ("snp", "wig", "disnp", "trisnp"):
                L.k4_free_host(getattr(f.files, k))
            L.k4_free_host(f.markers)
            L.k4_free_host(f.centroids)
            return dict(n_snps=f.files.n_snps, n_markers=f.n_markers, markers_bytes=f.markers_bytes, centroids_bytes=f.centroids_bytes)
        return fn

    forms = [("plain", plain)]
    if has2:
        forms += [("centroids", run2(0, True)), ("markers", run2(a.marker_len, False))]
    rep = dict(seqs=a.seqs, seq_len=a.seq_len, read_len=READ_LEN, coverage=a.coverage, reads=n, marker_len=a.marker_len, reps=a.reps,
               device=torch.cuda.get_device_name(0), runs={})
    for name, fn in forms:
        fn()  # warm-up (allocations, code objects)
        secs = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            secs.append(time.perf_counter() - t0)
        rep["runs"][name] = dict(s_median=float(np.median(secs)), s_min=min(secs), s_max=max(secs), s=secs, out=out)
        print(name, json.dumps(rep["runs"][name]), flush=True)
    if has2:
        for name in ("centroids", "markers"):
            rep["runs"][name]["added_s"] = rep["runs"][name]["s_median"] - rep["runs"]["plain"]["s_median"]
    ix.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rep, open(a.out, "w"), indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
