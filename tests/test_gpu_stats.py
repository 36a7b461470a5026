"""kalign's alignment statistics files (`-O`) on the device: `k4align -O` writes, byte for byte, the three files `ngskit4b kalign -O`
wrote (tests/golden/make_golden_stats.py) and its SAM stays the reference's SAM; SfxIndex.align_stats equals the literal
restatement (tests/stats_ref.py) array for array on ~2 M synthetic alignments (mixed lengths, one read longer than the kernel's
LDS table, both strands, trims, four quality bands, two-segment and rejected reads) and on an index of 12 000 sequences (the
per-target path without the LDS table)."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import stats_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
K4ALIGN = os.path.join(os.path.dirname(HERE), "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "stats_cases.json")))


def _unxz(tmp_path, name):
    dst = str(tmp_path / name[:-3])
    open(dst, "wb").write(lzma.open(os.path.join(GOLDEN, name)).read())
    return dst


def _golden(case, key):
    p = os.path.join(GOLDEN, "stats_%s.%s.xz" % (case, key))
    return lzma.open(p).read() if os.path.exists(p) else None


def _sam(text):
    return [l for l in text.split("\n") if l and not l.startswith("@PG")]


@pytest.mark.parametrize("case", sorted(CASES))
def test_k4align_writes_the_reference_files(tmp_path, case):
    meta = CASES[case]
    sfx = os.path.join(GOLDEN, "g1.sfx") if meta["index"] == "g1" else _unxz(tmp_path, meta["index"] + ".sfx.xz")
    files = []
    for flag, r in zip(("-i", "-u"), meta["reads"]):
        files += [flag, _unxz(tmp_path, r)]
    out, st = str(tmp_path / "o.sam"), str(tmp_path / "o.stats.csv")
    p = subprocess.run([K4ALIGN, "-I", sfx, "-o", out, "-O", st] + meta["args"] + files, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    for name, n in meta["nar"].items():
        assert ("%d (%s)" % (n, name)) in p.stderr, (name, n)
    got = {"main": st, "cnts": str(tmp_path / "o.stats.AlignCntsDist.csv"), "peins": str(tmp_path / "o.stats.GlobalPEInsertDist.csv")}
    for key, path in got.items():
        want = _golden(case, key)
        if want is None:
            assert not os.path.exists(path), key
        else:
            assert os.path.exists(path), key
            assert open(path, "rb").read() == want, key
    # the stage leaves the results alone: the SAM is the reference's, and the one of the run without -O
    assert _sam(open(out).read()) == _sam(_golden(case, "sam").decode())
    out2 = str(tmp_path / "plain.sam")
    p = subprocess.run([K4ALIGN, "-I", sfx, "-o", out2] + meta["args"] + files, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and open(out2, "rb").read() == open(out, "rb").read()


def test_a_failed_run_leaves_no_statistics_file(tmp_path):
    st = str(tmp_path / "x.csv")
    p = subprocess.run([K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-o", str(tmp_path / "o.sam"), "-O", st, "-i", str(tmp_path / "missing.fa")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and not os.path.exists(st)


# ---- the device entry point on synthetic alignments -----------------------------------------------------------------------------
def synthetic(chroms, n, seed, long_read=0, min_len=50, max_len=150):
    """n alignments over `chroms` as device-layout arrays (reads, offs, lens, rr, hits) and as restatement records: reads cut from
    the genome on either strand with ~2 % substitutions, random 4-bit quality scores (all four bands), an N among the first three
    bases of ~1 %, trims at either end of ~15 %, ~3 % two-segment hits, ~8 % rejected reads; long_read: length of read 0"""
    import kit4b_amd

    rng = np.random.default_rng(seed)
    clens = np.array([len(c) for c in chroms], np.int64)
    base = np.concatenate([[0], np.cumsum(clens)])[:-1]
    concat = np.concatenate([np.asarray(c, np.uint8) for c in chroms])
    ok = np.flatnonzero(clens >= min_len)
    chrom = ok[rng.integers(0, len(ok), n)]
    lens = np.minimum(rng.integers(min_len, max_len + 1, n), clens[chrom]).astype(np.int64)
    if long_read:
        chrom[0], lens[0] = int(np.argmax(clens)), long_read
    start = (rng.random(n) * (clens[chrom] - lens + 1)).astype(np.int64)
    minus = rng.random(n) < 0.5
    offs = np.concatenate([[0], np.cumsum(lens)])
    tot = int(offs[-1])
    rid = np.repeat(np.arange(n, dtype=np.int32), lens)
    pos = np.arange(tot, dtype=np.int64) - offs[rid]
    g = base[chrom][rid] + np.where(minus[rid], (start + lens - 1)[rid] - pos, start[rid] + pos)
    b = concat[g]
    b = np.where(minus[rid] & (b < 4), 3 - b, b).astype(np.uint8)
    sub = (rng.random(tot) < 0.02) & (b < 4)
    b[sub] = (b[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    n_first = np.flatnonzero(rng.random(n) < 0.01)
    b[offs[n_first] + rng.integers(0, 3, len(n_first))] = 4
    reads = (b | (rng.integers(0, 16, tot).astype(np.uint8) << 4)).astype(np.uint8)
    tl = np.where(rng.random(n) < 0.15, rng.integers(0, 20, n), 0)
    tr = np.where(rng.random(n) < 0.15, rng.integers(0, 20, n), 0)
    segs = rng.random(n) < 0.03
    nar = np.where(rng.random(n) < 0.08, rng.integers(2, 9, n), 1)
    rr = np.zeros(n, kit4b_amd.RESULT_DTYPE)
    rr["nar"], rr["num_hits"], rr["hit_rslt"], rr["inst"] = nar, nar == 1, 1, 1
    hits = np.zeros(n, kit4b_amd.HIT_DTYPE)
    hits["chrom_id"], hits["match_loci"], hits["match_len"] = chrom + 1, start, lens
    hits["strand"] = np.where(minus, ord("-"), ord("+"))
    hits["reserved"] = tl | (tr << 12) | np.where(segs, 1 << 25, 0)
    recs = [dict(nar=int(nar[i]), chrom=int(chrom[i]) + 1, loci=int(start[i]), mlen=int(lens[i]), strand="-" if minus[i] else "+",
                 tl=int(tl[i]), tr=int(tr[i]), segs=bool(segs[i]), read=reads[offs[i]:offs[i + 1]]) for i in range(n)]
    return dict(reads=reads, offs=offs[:-1].astype(np.uint64), lens=lens.astype(np.uint32), rr=rr, hits=hits, recs=recs)


def check_equal(ix, s, chroms):
    import torch

    n, max_len = len(s["lens"]), int(s["lens"].max())
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()  # noqa: E731
    d_reads = torch.cat([dev(s["reads"]), torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d = {k: dev(s[k]) for k in ("offs", "lens", "rr", "hits")}
    got = ix.align_stats(n, 1, max_len, d_reads, d["offs"], d["lens"], d_rr=d["rr"], d_hits=d["hits"])
    want = stats_ref.collect(s["recs"], [np.asarray(c, np.uint8) for c in chroms], max_len)
    assert got["n_accepted"] == want["n_accepted"] > 0.8 * n
    assert got["max_align_len"] == want["max_align_len"] == max_len
    for k in ("q_insts", "q_subs", "m_sub", "ent_hits", "ent_uniq_loci", "ent_indeterminate", "ent_trimer"):
        assert np.array_equal(got[k], want[k]), k
    assert not got["multi_hit"].any() and not got["pe_len_dist"].any()  # the run tallies were not collected
    assert np.array_equal(d["rr"].cpu().numpy(), s["rr"].view(np.uint8)) and np.array_equal(d["hits"].cpu().numpy(), s["hits"].view(np.uint8))
    return got


def test_device_counts_equal_the_restatement_2m_reads():
    import kit4b_amd
    import synth

    kit4b_amd.lib()
    _, chroms = synth.golden_genome()
    ix = kit4b_amd.SfxIndex.open(os.path.join(GOLDEN, "g1.sfx"))
    try:
        s = synthetic(chroms, 2_000_000, 0x57B1, long_read=1500)  # (1500 > the 1024 positions of the kernel's LDS table)
        got = check_equal(ix, s, chroms)
        assert all(got["q_insts"][b].sum() > 10_000_000 for b in range(4))  # every quality band is live
        assert got["q_insts"][:, 1024:].sum() > 0 and got["q_subs"].sum() > 1_000_000
    finally:
        ix.close()


def test_device_counts_equal_the_restatement_12000_targets():
    import torch

    import kit4b_amd as k4

    k4.lib()
    rng = np.random.default_rng(0x57B2)
    n_chrom = 12_000
    clens = rng.integers(120, 400, n_chrom)
    chroms = [rng.integers(0, 4, int(ln)).astype(np.uint8) for ln in clens]
    seq = np.concatenate([np.concatenate([c, [7]]) for c in chroms]).astype(np.uint8)
    d_seq = torch.from_numpy(seq).cuda()
    sa = torch.empty(len(seq), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(seq), 4, d_seq.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(len(seq), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(["t%05d" % i for i in range(n_chrom)], clens),
                                 keep=(sa, d_seq))
    try:
        s = synthetic(chroms, 300_000, 0x57B3, min_len=50, max_len=110)
        s["recs"] = [r for r in s["recs"]]
        got = check_equal(ix, s, chroms)
        assert (got["ent_hits"] > 0).sum() > 11_000
    finally:
        ix.close()
