"""kalign's PCR artefact reduction (`-k`) without a GPU: the restatement in tests/pcrdup_ref.py against what the reference binary
did (tests/golden/make_golden_pcrdup.py), and the argument rules of `k4align -k`."""
import json
import lzma
import os
import subprocess
import sys

import pytest

import pcrdup_ref
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)
K4ALIGN = os.path.join(ROOT, "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "pcrdup_cases.json")))
DP_NAMES = json.load(lzma.open(os.path.join(GOLDEN, "pcrdup_dp_names.json.xz"), "rt"))
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def _genome(index):
    if index == "g1":
        return synth.golden_genome()[1]
    sys.path.insert(0, GOLDEN)
    from make_golden_ext import genome

    return genome()[1]


def base_records(name):
    """the accepted alignments of the case's run without -k, as restatement records in load order (read names rd<load order>):
    AdjStartLoci = POS - 1, AdjHitLen = the M bases, LowMMCnt = the mismatches over them"""
    meta = CASES[name]
    chroms = _genome(meta["index"])
    text = lzma.open(os.path.join(GOLDEN, meta["base"]), "rt").read().splitlines()
    sq = [[f[3:] for f in l.split("\t") if f.startswith("SN:")][0] for l in text if l.startswith("@SQ")]
    recs = []
    for l in text:
        if l.startswith("@"):
            continue
        f = l.split("\t")
        cig = f[5]
        num = ""
        clip_l, m = 0, 0
        for ch in cig:
            if ch.isdigit():
                num += ch
                continue
            if ch == "S" and m == 0:
                clip_l = int(num)
            elif ch == "M":
                m += int(num)
            else:
                assert ch == "S", cig
            num = ""
        start = int(f[3]) - 1
        c = sq.index(f[2])
        ref = chroms[c][start:start + m]
        seq = f[9][clip_l:clip_l + m]
        mm = sum(1 for a, b in zip(seq, ref) if "ACGTN"[b] != a)
        recs.append(dict(name=f[0], load=int(f[0][2:]), nar=1, num_hits=1, chrom=c + 1, start=start, len=m,
                         strand="-" if int(f[1]) & 16 else "+", low_mm=mm))
    recs.sort(key=lambda r: r["load"])
    return recs


SE_CASES = [c for c in CASES if not c.startswith("pe_")]


@pytest.mark.parametrize("case", SE_CASES)
def test_restatement_predicts_the_reference_duplicates(case):
    """the restatement over the no-`-k` run's alignments marks exactly the reads the reference marked DP in the `-k` run"""
    meta = CASES[case]
    win = int([a for a in meta["args"] if a.startswith("-k")][0][2:])
    recs = base_records(case)
    assert len(recs) == meta["base_nar"]["AA"]
    n = pcrdup_ref.reduce_pcr_duplicates(recs, win)
    got = sorted(r["name"] for r in recs if r["nar"] == pcrdup_ref.NAR_PCRDUP)
    assert n == meta["nar"]["DP"] == len(DP_NAMES[case])
    assert got == DP_NAMES[case]
    assert n > 100


def test_golden_cases_reach_every_limit_bucket():
    """the k20 reads hold sites of every LimitDups value (1, 2, 3, 4, 5, 10, 50) with stacks deeper than the limit"""
    recs = base_records("k20_M1")
    sites = {}
    for r in recs:
        sites.setdefault((r["chrom"], r["strand"]), set()).add(r["start"])
    seen = set()
    import bisect

    for (c, s), st in sites.items():
        v = sorted(st)
        for x in v:
            up = bisect.bisect_left(v, x) - bisect.bisect_left(v, max(x - 20, 0))
            dn = bisect.bisect_right(v, x + 20) - bisect.bisect_right(v, x)
            seen.add(pcrdup_ref.limit_of(up, dn, 20))
    assert seen == {1, 2, 3, 4, 5, 10, 50}


def _k4align(*args):
    return subprocess.run([K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-o", "/dev/null", "-i", os.path.join(GOLDEN, "names.fa")] + list(args),
                          capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("k", ["-k-1", "-k251"])
def test_k_outside_its_range_exits_1(k):
    p = _k4align(k)
    assert p.returncode == 1 and "outside of range 0..250" in p.stderr and k in p.stderr


@pytest.mark.parametrize("extra", [["-b", "1"], ["-S", "0/2"], ["-G", "0"]])
def test_k_needs_the_whole_run(extra):
    p = _k4align("-k20", *extra)
    assert p.returncode == 1 and "-k reduces PCR duplicates over all reads of the run" in p.stderr


def test_k_with_r5_is_not_built():
    p = _k4align("-k20", "-r5", "-R8")
    assert p.returncode == 3 and "not built" in p.stderr
