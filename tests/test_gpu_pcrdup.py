"""kalign's PCR artefact reduction (`-k`) on the device: `k4align -k` writes what `ngskit4b kalign -k` wrote
(tests/golden/make_golden_pcrdup.py), and k4_reduce_pcr_dups_dev marks, read for read, what the literal restatement of
ReducePCRduplicates (tests/pcrdup_ref.py) marks on ~2 M synthetic results."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import pcrdup_ref
import samutil

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
K4ALIGN = os.path.join(os.path.dirname(HERE), "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "pcrdup_cases.json")))


def _unxz(tmp_path, name):
    dst = str(tmp_path / name[:-3])
    open(dst, "wb").write(lzma.open(os.path.join(GOLDEN, name)).read())
    return dst


def _files(tmp_path, rs):
    if rs == "p":
        return ["-i", _unxz(tmp_path, "pcrdup_p_1.fa.xz"), "-u", _unxz(tmp_path, "pcrdup_p_2.fa.xz")]
    return ["-i", _unxz(tmp_path, "pcrdup_%s.fa.xz" % rs)]


def _body(path):
    return [l for l in open(path).read().split("\n") if l and not l.startswith("@")]


def _header(path):
    return [l for l in open(path).read().split("\n") if l.startswith("@") and not l.startswith("@PG")]


@pytest.mark.parametrize("case", sorted(CASES))
def test_k4align_writes_the_reference_output(tmp_path, case):
    meta = CASES[case]
    sfx = os.path.join(GOLDEN, "g1.sfx") if meta["index"] == "g1" else _unxz(tmp_path, "g3.sfx.xz")
    out = str(tmp_path / ("o." + meta["out"]))
    p = subprocess.run([K4ALIGN, "-I", sfx, "-o", out] + meta["args"] + _files(tmp_path, meta["reads"]), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr
    for name, n in meta["nar"].items():
        assert ("%d (%s)" % (n, name)) in p.stderr, (name, n)
    if not case.startswith("pe_"):
        assert ("%d potential PCR artefact reads removed" % meta["nar"]["DP"]) in p.stderr
    if meta["out"] == "bam":
        text, refs, recs = samutil.read_bam(out)
        wtext, wrefs, wrecs = samutil.read_bam(os.path.join(GOLDEN, "pcrdup_%s.bam" % case))
        assert refs == wrefs
        assert [l for l in text.splitlines() if not l.startswith("@PG")] == [l for l in wtext.splitlines() if not l.startswith("@PG")]
        key = lambda r: (r["ref"], r["pos"], r["name"], r["flag"])  # noqa: E731
        assert sorted(recs, key=key) == sorted(wrecs, key=key) and len(recs) == meta["nar"]["AA"]
        return
    want = _unxz(tmp_path, "pcrdup_%s.sam.xz" % case)
    got = _body(out)
    assert _header(out) == _header(want)
    wbody = _body(want)
    n_acc = meta["nar"]["AA"]
    assert len(got) == len(wbody) and got[:n_acc] == wbody[:n_acc]  # the alignments: line for line
    if "-M1" in meta["args"]:  # the unaligned tail: the same NAR groups in the same order, each group as a set
        code = lambda l: samutil.NAR_CODES.index(l.rsplit("YU:Z:", 1)[1])  # noqa: E731
        assert [code(l) for l in got[n_acc:]] == [code(l) for l in wbody[n_acc:]]
        assert sorted(got[n_acc:]) == sorted(wbody[n_acc:])
        dp_names = json.load(lzma.open(os.path.join(GOLDEN, "pcrdup_dp_names.json.xz"), "rt"))[case]
        assert sorted(l.split("\t", 1)[0] for l in got if l.endswith("YU:Z:DP")) == dp_names
    if "-p5" in meta["args"]:
        assert open(out + ".snp", "rb").read() == lzma.open(os.path.join(GOLDEN, "pcrdup_%s.snp.xz" % case)).read()
    if case.startswith("pe_"):  # PE: -k is accepted and does nothing
        assert meta["nar"]["DP"] == 0
        out2 = str(tmp_path / "nok.sam")
        p = subprocess.run([K4ALIGN, "-I", sfx, "-o", out2] + [a for a in meta["args"] if not a.startswith("-k")] + _files(tmp_path, meta["reads"]),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and _body(out2) == got


# ---- the device entry point on synthetic results ------------------------------------------------------------------------------
def synthetic_results(n, seed):
    """(rr int32[n,6], hits int32[n,4]) in k4_read_result / k4_hit layout: random chromosomes, starts, strands, lengths, trims and
    low_mm; a 100 000-read stack at one locus, stacks at CurStart +- WinLen of one another, stacks near chromosome starts, stacked
    first and last sorted reads; ~8 % of the reads not accepted"""
    rng = np.random.default_rng(seed)
    clens = np.array([3000, 400000, 40_000_000, 120_000_000, 200_000_000, 80_000], np.int64)
    n_chrom = len(clens)
    chrom = rng.choice(n_chrom, n, p=clens / clens.sum()).astype(np.int64) + 1
    mlen = rng.integers(50, 151, n)
    start = (rng.random(n) * (clens[chrom - 1] - mlen)).astype(np.int64)
    strand = np.where(rng.random(n) < 0.5, ord("+"), ord("-"))
    tl = np.where(rng.random(n) < 0.1, rng.integers(0, 20, n), 0)
    tr = np.where(rng.random(n) < 0.1, rng.integers(0, 20, n), 0)
    low = rng.integers(0, 6, n)
    k = 0

    def put(m, c, s, st, L, t_l=0, t_r=0):  # m copies of one alignment from position k on
        nonlocal k
        sl = slice(k, k + m)
        chrom[sl], start[sl], strand[sl], mlen[sl], tl[sl], tr[sl] = c, s, ord(st), L, t_l, t_r
        k += m

    put(100_000, 3, 1_234_567, "+", 100)  # one big stack ...
    put(3000, 3, 1_234_567, "+", 120)  # ... with other lengths and the other strand at the same start
    put(2000, 3, 1_234_567, "-", 100)
    for W in (1, 7, 250):  # starts exactly at CurStart +- WinLen (AdjStartLoci = MatchLoci + TrimLeft for '+')
        for base in (5_000_000 + W * 1000, 6_000_000 + W * 1000):
            for d in (-W - 1, -W, 0, W, W + 1):
                put(int(rng.integers(2, 30)), 4, base + d - 3, "+", 90, 3, 0)
                put(int(rng.integers(2, 30)), 4, base + d, "-", 90, 0, 0)
    for c in range(1, n_chrom + 1):  # stacks and tilings at positions <= WinLen
        for s in range(0, 260, 3):
            put(int(rng.integers(1, 12)), c, s, "+" if s % 2 else "-", 60)
    for s in range(2_000_000, 2_000_300):  # a dense tiling: every LimitDups bucket
        put(int(rng.integers(1, 4)), 5, s, "+", 80)
    put(500, 1, 0, "+", 50)  # the first sorted read is stacked ...
    put(400, n_chrom, int(clens[-1]) - 151, "-", 150)  # ... and the last
    assert k < n
    nar = np.where(rng.random(n) < 0.92, 1, rng.choice([0, 2, 3, 4, 5, 6], n))
    nar[:k] = np.where(rng.random(k) < 0.97, 1, 3)
    order = rng.permutation(n)  # stacks spread over the load order
    chrom, start, strand, mlen, tl, tr, low, nar = (a[order] for a in (chrom, start, strand, mlen, tl, tr, low, nar))
    rr = np.zeros((n, 6), np.int32)
    rr[:, 0] = 1
    rr[:, 1] = np.where(nar == 1, 1, 0)
    rr[:, 2] = low
    rr[:, 3] = low + 1
    rr[:, 4] = nar
    rr[:, 5] = np.where(nar == 1, 1, np.where(nar == 5, 3, 0))
    hits = np.zeros((n, 4), np.int32)
    hits[:, 0] = chrom
    hits[:, 1] = start
    hits[:, 2] = (mlen | (strand << 16) | (low << 24)).astype(np.int64).astype(np.uint32).view(np.int32)
    hits[:, 3] = (tl | (tr << 12)).astype(np.int32)
    return rr, hits


def restate(rr, hits, win):
    h2 = hits[:, 2].view(np.uint32)
    mlen, strand = (h2 & 0xFFFF).astype(np.int64), ((h2 >> 16) & 0xFF).astype(np.int64)
    tl, tr = (hits[:, 3] & 0xFFF).astype(np.int64), ((hits[:, 3] >> 12) & 0xFFF).astype(np.int64)
    adj_start = hits[:, 1].astype(np.int64) + np.where(strand == ord("+"), tl, tr)
    adj_len = mlen - tl - tr
    recs = [dict(nar=int(a), num_hits=int(b), chrom=int(c), start=int(d), len=int(e), strand=chr(f), low_mm=int(g))
            for a, b, c, d, e, f, g in zip(rr[:, 4], rr[:, 5], hits[:, 0], adj_start, adj_len, strand, rr[:, 2])]
    n = pcrdup_ref.reduce_pcr_duplicates(recs, win)
    out = rr.copy()
    dp = np.array([r["nar"] == pcrdup_ref.NAR_PCRDUP for r in recs])
    out[dp, 4] = pcrdup_ref.NAR_PCRDUP
    out[dp, 5] = 0
    out[dp, 1] = 0
    return out, n


@pytest.fixture(scope="module")
def ix():
    import kit4b_amd

    kit4b_amd.lib()
    x = kit4b_amd.SfxIndex.open(os.path.join(GOLDEN, "g1.sfx"))
    yield x
    x.close()


@pytest.fixture(scope="module")
def synth_results():
    return synthetic_results(2_000_000, 0x9C10)


@pytest.mark.parametrize("win", [0, 1, 7, 250])
def test_device_stage_equals_the_restatement(ix, synth_results, win):
    import torch

    rr, hits = synth_results
    want, n_want = restate(rr, hits, win)
    d_rr, d_hits = torch.from_numpy(rr.copy()).cuda(), torch.from_numpy(hits.copy()).cuda()
    n = ix.reduce_pcr_dups(win, len(rr), 1, d_rr, d_hits, torch.cuda.current_stream().cuda_stream)
    got = d_rr.cpu().numpy()
    assert n == n_want and n > 100_000
    assert np.array_equal(got, want)
    assert np.array_equal(d_hits.cpu().numpy(), hits)  # the hits stay as they were


def test_device_stage_with_nothing_to_do(ix):
    import torch

    rr, hits = synthetic_results(200_000, 0x9C11)
    d_rr, d_hits = torch.from_numpy(rr.copy()).cuda(), torch.from_numpy(hits.copy()).cuda()
    assert ix.reduce_pcr_dups(20, 0, 1, d_rr, d_hits) == 0
    rr[:, 4] = np.where(rr[:, 4] == 1, 3, rr[:, 4])  # no accepted read
    d_rr = torch.from_numpy(rr.copy()).cuda()
    assert ix.reduce_pcr_dups(20, len(rr), 1, d_rr, d_hits) == 0
    assert np.array_equal(d_rr.cpu().numpy(), rr)
