"""kalign's 5' PCR primer correction (`-6 <n>`) without a GPU: the restatement (tests/primer_ref.py) applied to the reference's own
-M1 run at the inflated rate reproduces the reference's -6 run (tests/golden/make_golden_primer.py); k4align's argument rules, which
are decided before a device is opened; and the crafted inputs of tests/test_gpu_primer.py make the claims they are there for."""
import json
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

import primer_craft
import primer_ref
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
K4ALIGN = os.path.join(os.path.dirname(HERE), "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "primer_cases.json")))
MARKS = json.load(lzma.open(os.path.join(GOLDEN, "primer_marks.json.xz"), "rt"))


def _lines(name):
    return [l for l in lzma.open(os.path.join(GOLDEN, name), "rt").read().split("\n") if l and not l.startswith("@")]


@pytest.fixture(scope="module")
def genome():
    return synth.golden_genome()


# (seg_a12_A3000 is left to the GPU test: -A forces the flank autotrim, which runs behind the stage at the rate given with -s, so no
# command line of the reference shows the records the stage saw there)
@pytest.mark.parametrize("case", sorted(c for c in CASES if CASES[c]["restate"]))
def test_restatement_reproduces_the_reference(genome, case):
    meta = CASES[case]
    names, chroms = genome
    base = _lines(meta["base"])
    recs = primer_ref.sam_records(base, names, chroms)
    was_accepted = {r["key"] for r in recs if r["nar"] == 1}
    assert len(was_accepted) == meta["base_nar"]["AA"]
    totals = primer_ref.pcr5_primer_correct(recs, meta["subs"], primer_ref.genome_target(chroms))
    assert totals == meta["totals"]
    accepted = [r for r in recs if r["nar"] == 1]
    turned_nl = sorted(r["key"] for r in recs if r["nar"] == primer_ref.NAR_NOHIT)
    assert len(turned_nl) == meta["totals"][2]
    # the reads that are NL under -6: the stage's, and those the alignment at the inflated rate had left NL
    assert sorted(turned_nl + [r["key"] for r in recs if r.get("code") == "NL"]) == MARKS[case]
    if meta["out"] != "sam":  # (BAM and genpba: the same command line as s1_p3_M1 as far as the stage goes)
        assert len(accepted) == meta["nar"]["AA"]
        return
    want = _lines("primer_%s.sam.xz" % case)
    n_acc = sum(1 for l in want if "YU:Z:" not in l)
    key = lambda l: l.split("\t", 2)[0] + "/" + str((int(l.split("\t", 2)[1]) >> 7) & 1)  # noqa: E731
    seq_of = {key(l): l.split("\t")[9] for l in want[:n_acc]}
    if any(a.startswith("-x") for a in meta["args"]):
        # the flank autotrim runs behind the stage: it turns reads down (ET) and clips others; SEQ still shows the whole read
        assert set(seq_of) <= {r["key"] for r in accepted}
        assert all(primer_ref.sam_seq(r) == seq_of[r["key"]] for r in accepted if r["key"] in seq_of)
        return
    assert n_acc == len(accepted)
    if len(meta["reads"]) == 2:  # PE: the line of a read whose mate was rejected loses its mate fields; names and SEQ are compared
        assert {r["key"]: primer_ref.sam_seq(r) for r in accepted} == seq_of
        return
    # SE, line for line: SortHitMatch orders by (chrom, start, length, strand, LowMMCnt) and then load order, so a corrected read
    # moves among the reads of its position
    load = lambda r: int(re.sub(r"\D", "", r["key"].split("/")[0]) or 0)  # noqa: E731
    accepted.sort(key=lambda r: (r["chrom"], r["loci"], r["match_len"], r["strand"] == "-", r["low_mm"], load(r)))
    assert [primer_ref.sam_line(r) for r in accepted] == want[:n_acc]
    if "-M1" in meta["args"]:
        tail = sorted(l.split("\t")[0] + " " + l.split("\t")[9] + " " + l.rsplit("YU:Z:", 1)[1] for l in want[n_acc:])
        mine = sorted(r["key"].split("/")[0] + " " + primer_ref.sam_seq(r) + " " + ("NL" if r["nar"] == 3 else r["code"]) for r in recs if r["nar"] != 1)
        assert tail == mine  # a rejected read is reported as it was read


def test_golden_cases_cover_the_rules():
    assert all(m["totals"][0] > 0 and m["totals"][2] > 0 for c, m in CASES.items() if c != "s14_p5")
    assert any(m["totals"][1] > m["totals"][0] for m in CASES.values())
    assert CASES["s14_p5"]["base_subs"] == 15 and CASES["s14_p5"]["nar"] == CASES["s14_p5"]["base_nar"]
    assert any(any(c in l.split("\t")[5] for c in "NID") for l in _lines("primer_seg_a12_A3000.sam.xz"))
    assert CASES["s1_p3_k20_x5"]["nar"]["DP"] > 100
    assert primer_ref.initial_align_subs(14, 5) == 15 and primer_ref.initial_align_subs(1, 3) == 4 and primer_ref.initial_align_subs(3, 0) == 3


# ---- k4align: the rules are decided before the index is opened, so they run without a GPU -----------------------------------------
@pytest.fixture(scope="module")
def base(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("primer_opts")
    fa = tmp / "r.fa"
    fa.write_text(">r1\n" + "ACGT" * 25 + "\n")
    return [K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-i", str(fa)], tmp


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("opt", [["-6", "6"], ["-6-1"], ["--pcrprimersubs", "7"], ["--pcrprimersubs=9"]])
def test_out_of_range_exits_1_with_kaligns_text(base, opt):
    cmd, tmp = base
    p = run(cmd + ["-o", str(tmp / "o.sam")] + opt)
    n = int(re.sub(r"[^-\d]", "", "".join(opt)[2:]) if opt[0].startswith("-6") else re.sub(r"\D", "", "".join(opt)))
    assert p.returncode == 1 and ("PCR primer correction subs '-6%d' specified outside of range 0..5" % n) in p.stderr
    assert not os.path.exists(str(tmp / "o.sam"))


def test_chimeric_trimming_conflict_exits_1(base):
    cmd, tmp = base
    p = run(cmd + ["-o", str(tmp / "o.sam"), "-6", "2", "-c50"])
    assert p.returncode == 1 and "PCR primer correction subs not allowed when also specifying chimeric trimming" in p.stderr


def test_r5_is_not_built(base):
    cmd, tmp = base
    p = run(cmd + ["-o", str(tmp / "r5.sam"), "-6", "2", "-r5", "-R8"])
    assert p.returncode == 3 and "not built" in p.stderr and not os.path.exists(str(tmp / "r5.sam"))


@pytest.mark.parametrize("opt", [["-6", "0"], ["-60"], ["-6", "5"], ["--pcrprimersubs", "3"]])
def test_in_range_values_are_accepted(base, opt):
    """the option is taken (no usage text, no -6 message): the run ends at the next rule, an -s outside of its range; -6 0 with -c is
    no conflict either"""
    cmd, tmp = base
    p = run(cmd + ["-o", str(tmp / "o.sam"), "-s99"] + opt + (["-c50"] if opt[-1] in ("0", "-60") else []))
    assert p.returncode == 1 and "'-s99' specified outside of range 0..15" in p.stderr
    assert "PCR primer" not in p.stderr and "k4align -i" not in p.stderr


def test_genpba_takes_the_option(base):
    cmd, tmp = base
    p = run(cmd + ["-o", str(tmp / "o.pba"), "-M3", "--experimentid", "e1", "--readsetid", "r1", "-6", "3", "-s99"])
    assert p.returncode == 1 and "'-s99' specified outside of range 0..15" in p.stderr and "has no option" not in p.stderr


# ---- the crafted inputs of the GPU test -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_subs", [0, 1, 2, 5])
def test_crafted_inputs_make_their_claims(genome, max_subs):
    names, chroms = genome
    s = primer_craft.craft(chroms, 6000, 0x6A00 + max_subs)
    e = primer_craft.expected(s, max_subs, chroms)
    recs0, recs = s["recs"], e["recs"]
    n = len(recs0)
    acc = [i for i in range(n) if recs0[i]["nar"] == 1]
    for strand in "+-":
        idx = [i for i in acc if recs0[i]["strand"] == strand]
        assert sum(e["fixed"][i] > 0 for i in idx) > 20 and sum(recs[i]["nar"] == 3 for i in idx) > 20, strand
    assert {int(x) for x in s["lens"]} == set(primer_craft.LENS)
    if max_subs:  # 99 and 101 bp fall on either side of the rounding of (s * len + 50) / 100, or 50 and 150 bp do
        assert len({(max_subs * ln + 50) // 100 for ln in primer_craft.LENS}) >= 2
    assert {recs0[i]["planted"][0] for i in acc} == {0, 1, 2, 3, 4} and {recs0[i]["planted"][1] for i in acc} == set(range(7))
    assert any(11 in recs0[i]["front"] and e["fixed"][i] for i in acc) and any(12 in recs0[i]["back"] and recs[i]["nar"] == 1 for i in acc)
    for k in (1, 2, 3):
        assert sum(e["fixed"][i] == k for i in acc) > 5, k
    # a read whose later mismatches among the 12 stay: corrected, yet its first 12 still differ from the target
    tg = primer_ref.genome_target(chroms)

    def facing(r):
        t = tg(r["chrom"], r["loci"], r["read_len"])
        return (primer_ref.reverse_complement(t) if r["strand"] == "-" else t)[:12]

    assert max_subs == 0 or any(e["fixed"][i] and [b & 7 for b in recs[i]["seq"][:12]] != facing(recs[i]) for i in acc)
    assert e["totals"][2] > 100 and e["totals"][1] > e["totals"][0] > 100
    lens_of = [len(c) for c in chroms]
    assert any(r["strand"] == "+" and r["loci"] == 0 and e["fixed"][i] for i, r in enumerate(recs0))
    assert any(r["strand"] == "-" and r["loci"] + r["read_len"] == lens_of[r["chrom"] - 1] and e["fixed"][i] for i, r in enumerate(recs0))
    assert any(r["chrom"] == 4 and e["fixed"][i] for i, r in enumerate(recs0)) and any(r["chrom"] == 5 and e["fixed"][i] for i, r in enumerate(recs0))
    assert any(4 in facing(r) and r["nar"] == 1 and e["fixed"][i] for i, r in enumerate(recs0)), "an N in the target is written into the read"
    assert any(4 in [b & 7 for b in r["seq"][:12]] and e["fixed"][i] for i, r in enumerate(recs0)), "an N in the read is corrected"
    # the records the stage has to pass over, each kind holding reads over the rate
    over = lambda r: r["low_mm"] > (max_subs * r["read_len"] + 50) // 100  # noqa: E731
    for kind in (lambda r: r["nar"] != 1, lambda r: r["two_seg"] and r["nar"] == 1, lambda r: r["match_len"] != r["read_len"] and r["nar"] == 1):
        idx = [i for i, r in enumerate(recs0) if kind(r) and over(r)]
        assert len(idx) > 10 and all(recs[i]["nar"] == recs0[i]["nar"] and recs[i]["seq"] == recs0[i]["seq"] for i in idx)
    # only bits 0..2 of the first 12 bytes of a corrected read change
    diff = np.flatnonzero(e["reads"] != s["reads"])
    assert len(diff) == e["totals"][1] and np.all((e["reads"][diff] ^ s["reads"][diff]) < 8)
    rid = np.searchsorted(s["offs"], diff, side="right") - 1
    assert np.all(diff - s["offs"][rid].astype(np.int64) < 12)
    # a second pass finds nothing to do
    again = primer_craft.expected(dict(s, recs=recs), max_subs, chroms)
    assert again["totals"][:2] == [0, 0] and again["totals"][2] == 0
