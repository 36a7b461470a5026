"""kalign's loci base constraints (`-5`) and chromosome filters (`-Z` / `-z`) without a GPU: the restatement in tests/filter_ref.py,
applied to the reference's UNFILTERED -M1 SAM of every golden case (tests/golden/make_golden_filter.py), marks exactly the reads the
reference marked LC / FC / DP and arrives at its NAR counts and -- for the -M1 cases -- its SAM; the dense form of the restatement
equals the literal one; the CSV rules; the argument rules of k4align that need no device."""
import json
import lzma
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import filter_ref
import pcrdup_ref
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)
K4ALIGN = os.path.join(ROOT, "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "filter_cases.json")))
MARKS = json.load(lzma.open(os.path.join(GOLDEN, "filter_marks.json.xz"), "rt"))
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
NAR_CODES = ["NA", "AA", "EN", "NL", "MH", "ML", "ET", "OJ", "OM", "DP", "DS", "FC", "PR", "UI", "OI", "UP", "IS", "IT", "NP", "LC"]
G1_NAMES, G1_LENS = ["chr1", "chr2", "chr3", "chr4", "chr5"], [60000, 40000, 25000, 300, 120]


def genome(index):
    if index == "g1":
        return synth.golden_genome()
    sys.path.insert(0, GOLDEN)
    from make_golden_ext import genome as g3

    names, chroms, _, _ = g3()
    return names, chroms


def base_records(meta, untrim=False):
    """every record of the case's unfiltered -M1 run, in file order, as restatement records (PE: mates made neighbours); the key
    of a read is <name>/<0 PE1 or SE | 1 PE2>"""
    text = lzma.open(os.path.join(GOLDEN, meta["base"]), "rt").read().splitlines()
    sq = [[f[3:] for f in l.split("\t") if f.startswith("SN:")][0] for l in text if l.startswith("@SQ")]
    recs = []
    for l in text:
        if l.startswith("@"):
            continue
        f = l.split("\t")
        flag = int(f[1])
        r = dict(key="%s/%d" % (f[0], (flag >> 7) & 1), line=l, nar=1, num_hits=1, inst=1)
        if "YU:Z:" in f[-1]:
            r["nar"] = NAR_CODES.index(f[-1][5:])
            r["num_hits"] = 0
        else:
            ops = [(int(n), o) for n, o in re.findall(r"(\d+)([A-Z])", f[5])]
            minus = bool(flag & 16)
            lead = ops[0][0] if ops[0][1] == "S" else 0
            trail = ops[-1][0] if ops[-1][1] == "S" else 0
            # Seg[0]: the walk of the read starts at TrimLeft on either strand -- the trailing clip of a '-' alignment's SAM line
            # untrim: the flank autotrim (-x, forced by -A) runs BEHIND the constraints, which therefore saw the whole read
            if untrim and lead + trail:
                ops = [(n, o) for n, o in ops if o != "S"]
                ops[0] = (ops[0][0] + lead, "M")
                ops[-1] = (ops[-1][0] + trail, "M")
                f[3], lead, trail = str(int(f[3]) - lead), 0, 0
            loci, q, segs = int(f[3]) - 1, (trail if minus else lead), []
            for n, o in ops:
                if o == "M":
                    segs.append([loci, n, q])
                    loci, q = loci + n, q + n
                elif o in "DN":
                    loci += n
                elif o == "I":
                    q += n
            if len(segs) > 1:  # Seg[1].ReadOfs counts from the read's first base
                segs[1][2] = segs[1][2] - (trail if minus else lead) + lead
            start, m = int(f[3]) - 1, segs[0][1]
            r.update(chrom=sq.index(f[2]) + 1, strand="-" if minus else "+", seq=[CODE[c] for c in f[9]], segs=[tuple(s) for s in segs],
                     start=start, len=m, load=int(re.sub(r"\D", "", f[0]) or 0))
        recs.append(r)
    return recs


def restate(case):
    meta = CASES[case]
    names, chroms = genome(meta["index"])
    recs = base_records(meta, untrim=any(a.startswith("-A") for a in meta["args"]))
    pe = len(meta["reads"]) == 2
    if pe:  # mates side by side
        by = {}
        for r in recs:
            by.setdefault(r["key"][:-2], {})[r["key"][-1]] = r
        recs = [m[k] for m in by.values() for k in "01"]
    table = filter_ref.load_constraints(open(os.path.join(GOLDEN, meta["loci"])).read(), names, [len(c) for c in chroms]) if meta["loci"] else []
    counts = dict(LC=filter_ref.mark_loci_constraints(recs, table, lambda c, p: int(chroms[c - 1][p]), pe=pe))
    counts["DP"] = 0
    win = [int(a[2:]) for a in meta["args"] if a.startswith("-k")]
    if win and not pe:  # ReducePCRduplicates sits between the two stages
        acc = [r for r in recs if r["nar"] == 1]
        for r in acc:
            lo = r["segs"][0]
            mm = sum(1 for j in range(lo[1]) if r["seq"][lo[2] + j] != int(chroms[r["chrom"] - 1][lo[0] + j]))
            r["low_mm"] = mm
        acc.sort(key=lambda r: r["load"])
        counts["DP"] = pcrdup_ref.reduce_pcr_duplicates(acc, win[0])
    counts["FC"] = filter_ref.mark_chroms(recs, filter_ref.chrom_accept(names, meta["include"], meta["exclude"])) if meta["include"] or meta["exclude"] else 0
    return meta, recs, counts


# (lc_x5_excl is left to the GPU test: -x5 turns reads down between the two stages, and the flank autotrim is not restated here)
@pytest.mark.parametrize("case", sorted(c for c in CASES if "-x5" not in CASES[c]["args"]))
def test_restatement_reproduces_the_reference(case):
    meta, recs, counts = restate(case)
    pe = len(meta["reads"]) == 2
    if not pe:  # (PE: the mate of a marked read is marked whatever its state)
        assert sum(r["nar"] == 1 for r in recs) + counts["LC"] + counts["DP"] + counts["FC"] == meta["base_nar"]["AA"]
    if any(a.startswith(("-a", "-A")) for a in meta["args"]) and meta["base_nar"].get("OJ", 0) + meta["base_nar"].get("OM", 0):
        # The orphan junction / microInDel filters run BEHIND the constraints and look at the other reads: the unfiltered run dropped
        # reads as OJ / OM that the filtered run had marked LC before, and reads whose supporters became LC are orphans there.  What
        # can be said from this base: every read marked here is marked by the reference, and the rest were OJ / OM in the base run.
        mine = {r["key"] for r in recs if r["nar"] == 19}
        base_orphans = {r["key"] for r in recs if r["nar"] in (7, 8)}
        assert mine <= set(MARKS[case]["LC"]) and set(MARKS[case]["LC"]) - mine <= base_orphans and len(mine) > 100
        return
    for code, nar in (("LC", 19), ("FC", 11), ("DP", 9)):
        assert counts[code] == meta["nar"].get(code, 0), code
        assert sorted(r["key"] for r in recs if r["nar"] == nar) == MARKS[case][code], code
    assert sum(r["nar"] == 1 for r in recs) == meta["nar"]["AA"]
    for k, code in enumerate(NAR_CODES):  # the whole histogram (PE: -M1 lists the reads, the histogram of a PE run counts otherwise)
        assert pe or sum(r["nar"] == k for r in recs) == meta["nar"].get(code, 0), code
    if "-M1" in meta["args"]:  # the filtered SAM itself: the surviving alignments in the base run's order, then the marked reads
        want = [l for l in lzma.open(os.path.join(GOLDEN, "filter_%s.sam.xz" % case), "rt").read().splitlines() if not l.startswith("@")]
        n_acc = meta["nar"]["AA"]
        base_lines = [l for l in lzma.open(os.path.join(GOLDEN, meta["base"]), "rt").read().splitlines() if not l.startswith("@")]
        alive = {r["line"] for r in recs if r["nar"] == 1}
        kept = [l for l in base_lines[:meta["base_nar"]["AA"]] if l in alive]
        if len(meta["reads"]) == 1:
            assert kept == want[:n_acc]
        else:  # (a pair one of whose mates was marked: the survivor's mate fields change)
            assert len(kept) == n_acc == len(want) - sum(1 for l in want if "YU:Z:" in l)
        tail = sorted(l.split("\t")[0] + l.rsplit("\t", 1)[1] for l in want[n_acc:])
        names_of = {19: "LC", 11: "FC", 9: "DP"}
        mine = sorted(r["line"].split("\t")[0] + "YU:Z:" + (names_of.get(r["nar"]) or r["line"].rsplit("YU:Z:", 1)[1]) for r in recs if r["nar"] != 1)
        assert tail == mine


def test_golden_cases_cover_the_rules():
    lc = {c: restate(c) for c in ("lc_c50", "lc_seg_a12_A3000", "lc_a")}
    # a '-' alignment trimmed differently at its two ends that a constraint overlaps; a two-segment read; an N in a read
    recs = lc["lc_c50"][1]
    assert any(r.get("strand") == "-" and r["segs"][0][2] != len(r["seq"]) - r["segs"][0][1] - r["segs"][0][2] and r["nar"] == 19 for r in recs if "segs" in r)
    assert any(len(r["segs"]) == 2 for r in lc["lc_seg_a12_A3000"][1] if "segs" in r)
    table = filter_ref.load_constraints(open(os.path.join(GOLDEN, "filter_lc_a.csv")).read(), G1_NAMES, G1_LENS)
    assert len(table) == 4 and table[1][:3] == (1, 5000, 6000)  # the title line is sloughed; two constraints over chr1 5000-6000
    assert table == [c for c in filter_ref.load_constraints(open(os.path.join(GOLDEN, "filter_lc_b.csv")).read(), G1_NAMES, G1_LENS) if c[0] != 4 and c[1:3] != (0, 0)]


def test_dense_restatement_equals_the_literal_one():
    rng = np.random.default_rng(0xF117)
    names, chroms = synth.golden_genome()
    chroms = [np.asarray(c, np.uint8).copy() for c in chroms]
    chroms[3][10:20] = 4
    table = []
    for _ in range(60):
        c = int(rng.integers(1, 6))
        s = int(rng.integers(0, len(chroms[c - 1])))
        e = min(len(chroms[c - 1]) - 1, s + int(rng.integers(0, 400)))
        table.append((c, s, e, int(rng.integers(1, 32))))
    table += [(4, 0, 0, 16), (4, 299, 299, 1), (5, 119, 119, 16)]
    table.sort(key=lambda c: c[:3])
    n = 3000
    chrom = rng.integers(1, 6, n)
    lens = np.minimum(rng.integers(50, 120, n), [len(chroms[c - 1]) for c in chrom]).astype(np.int64)
    start = (rng.random(n) * (np.array([len(chroms[c - 1]) for c in chrom]) - lens + 1)).astype(np.int64)
    minus = rng.random(n) < 0.5
    tl, tr = rng.integers(0, 12, n), rng.integers(0, 12, n)
    offs = np.concatenate([[0], np.cumsum(lens)])
    reads = np.zeros(int(offs[-1]), np.uint8)
    recs = []
    for i in range(n):
        t = chroms[chrom[i] - 1][start[i]:start[i] + lens[i]].copy()
        mut = rng.random(lens[i]) < 0.05
        t[mut] = rng.integers(0, 5, int(mut.sum()))
        rd = synth.revcomp(t) if minus[i] else t
        reads[offs[i]:offs[i + 1]] = rd | (rng.integers(0, 16, lens[i]) << 4).astype(np.uint8)
        first = start[i] + (tr[i] if minus[i] else tl[i])
        recs.append(dict(nar=1 if rng.random() < 0.9 else 3, num_hits=1, chrom=int(chrom[i]), strand="-" if minus[i] else "+", seq=t,
                         segs=[(int(first), int(lens[i] - tl[i] - tr[i]), int(tl[i]))]))
    acc = np.array([r["nar"] == 1 for r in recs])
    seg_first = np.stack([start + np.where(minus, tr, tl), np.zeros(n, np.int64)])
    seg_n = np.stack([lens - tl - tr, np.zeros(n, np.int64)])
    seg_q = np.stack([tl, np.zeros(n, np.int64)])
    got = filter_ref.violations_dense(table, chroms, chrom, seg_first, seg_n, seg_q, minus, reads, offs[:-1], lens, acc)
    want = np.array([not filter_ref.accepts(r, table, lambda c, p: int(chroms[c - 1][p])) for r in recs])
    assert np.array_equal(got, want) and 100 < want.sum() < n - 100


@pytest.mark.parametrize("text,msg", [
    ("chr1,10,20\n", "Expected at least 4 fields at line 1"),
    ("chrom,start,end,bases\nchr9,10,20,A\n", "Unable to find matching indexed identifier for 'chr9' at line 2"),
    ("chr1,30,20,A\n", "Start loci must be >= 0 and <= end loci for 'chr1' at line 1"),
    ("chr1,-1,20,A\n", "Start loci must be >= 0"),
    ("chr4,10,300,A\n", "End loci must be > targeted sequence length for 'chr4' at line 1"),
    ("chr1,10,20,AX\n", "Illegal base specifiers for 'chr1' at line 1"),
    ("chr1,10,20, \n", "Illegal base specifiers"),
    ("".join("chr1,%d,%d,A\n" % (k, k) for k in range(6401)), "Number of constrained loci would be more than max (6400)"),
], ids=["fields", "name", "order", "negative", "length", "bases", "blank", "count"])
def test_constraint_file_errors(text, msg):
    with pytest.raises(filter_ref.ConstraintError, match=re.escape(msg)):
        filter_ref.load_constraints(text, G1_NAMES, G1_LENS)


def test_chrom_accept_rules():
    a = filter_ref.chrom_accept(G1_NAMES, exclude=["chr[45]"])
    assert a == [False, True, True, True, False, False]
    assert filter_ref.chrom_accept(G1_NAMES, include=["chr[12]$"], exclude=["chr2"]) == [False, True, False, False, False, False]  # exclude wins
    assert filter_ref.chrom_accept(["chr1 extra text", "x"], include=["text"]) == [False, False, False]  # the name ends at its first blank


# ---- k4align: what it decides before it touches a device -----------------------------------------------------------------------------
def _k4align(*args):
    return subprocess.run([K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-o", "/dev/null", "-i", os.path.join(GOLDEN, "names.fa")] + list(args),
                          capture_output=True, text=True, timeout=60)


LC = os.path.join(GOLDEN, "filter_lc_3.csv")


@pytest.mark.parametrize("extra", [["--chromexclude", "chr4", "-u", os.path.join(GOLDEN, "names.fa")], ["--chromeinclude=chr1", "-r5", "-R8"],
                                   ["-5", LC, "-r5", "-R8"], ["--lociconstraints", LC, "-r5", "-R8"]])
def test_combinations_that_are_not_built_exit_3(extra):
    p = _k4align(*extra)
    assert p.returncode == 3 and "not built" in p.stderr


def test_a_bad_expression_is_a_parameter_error():
    p = _k4align("--chromexclude", "chr[4")
    assert p.returncode == 1 and "Unable to compile exclusion regular expression 'chr[4'" in p.stderr
    assert _k4align("--chromeinclude", "(").returncode == 1
    assert _k4align("--nosuchoption", "x").returncode == 1 and _k4align("--chromexclude").returncode == 1


def test_a_missing_constraints_file_exits_2(tmp_path):
    p = _k4align("-5", str(tmp_path / "missing.csv"))
    assert p.returncode == 2 and "Unable to open" in p.stderr
