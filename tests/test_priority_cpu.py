"""kalign's priority regions (`-B <bed>`, `-V`) without a GPU: the restatement in tests/priority_ref.py -- the BED reader's interval
rules, the select rule over two AlignRead passes of the oracle, the filter -- places and marks every read of the single-end goldens
(tests/golden/make_golden_priority.py) as the reference did; and the argument rules of k4align that need no device."""
import json
import lzma
import os
import subprocess
import sys

import numpy as np
import pytest

import priority_ref
from oracle_bindings import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)
K4ALIGN = os.path.join(ROOT, "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "priority_cases.json")))
NAR_CODES = ["NA", "AA", "EN", "NL", "MH", "ML", "ET", "OJ", "OM", "DP", "DS", "FC", "PR", "UI", "OI", "UP", "IS", "IT", "NP", "LC"]
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
# the cases the two plain AlignRead passes decide: single end, default multiloci mode, no optional phase
PLAIN = [c for c in sorted(CASES) if len(CASES[c]["reads"]) == 1 and not any(a[:2] in ("-r", "-a", "-A", "-c") for a in CASES[c]["args"]) and
         "-M1" in CASES[c]["args"]]


def fasta(name):
    names, seqs = [], []
    for line in lzma.open(os.path.join(GOLDEN, name), "rt"):
        if line.startswith(">"):
            names.append(line[1:].split()[0])
            seqs.append("")
        else:
            seqs[-1] += line.strip()
    return names, seqs


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    sfx = str(tmp_path_factory.mktemp("priority") / "priority.sfx")
    open(sfx, "wb").write(lzma.open(os.path.join(GOLDEN, "priority.sfx.xz")).read())
    O = Oracle()
    h = O.open(sfx)
    O.set_max_iter(h, 5000)
    yield O, h, [e["name"] for e in O.entries(h)]
    O.close(h)


def golden_reads(case):
    """read name -> 'PR' / 'ML' / ... or (sequence, 1-based position, strand) of the reference's -M1 SAM"""
    got = {}
    for l in lzma.open(os.path.join(GOLDEN, "priority_%s.sam.xz" % case), "rt"):
        if l.startswith("@"):
            continue
        f = l.rstrip("\n").split("\t")
        got[f[0]] = f[-1][5:] if f[-1].startswith("YU:Z:") else (f[2], int(f[3]), "-" if int(f[1]) & 16 else "+")
    return got


@pytest.mark.parametrize("case", PLAIN)
def test_restatement_places_every_read_as_the_reference(oracle, case):
    O, h, index_names = oracle
    meta = CASES[case]
    args = meta["args"]
    names, seqs = fasta("priority_%s.fa.xz" % meta["reads"][0])
    reads = [np.array([CODE[c] for c in s], np.uint8) for s in seqs]
    kw = dict(max_subs=int([a[2:] for a in args if a.startswith("-s")][0]), min_edit_dist=int(([a[2:] for a in args if a.startswith("-e")] + ["1"])[0]))
    norm = O.kalign_batch(h, reads, max_ml=1, **kw)
    out, hits = norm["out"], norm["hits"]
    regions = None
    if meta["bed"]:
        regions = priority_ref.Regions(open(os.path.join(GOLDEN, "priority_%s.bed" % meta["bed"])).read(), index_names)
        wide = O.kalign_batch(h, reads, max_ml=1 + priority_ref.PRIORITY_EXACTS, **kw)
        out, hits, need = priority_ref.select(regions, wide["out"], wide["hits"], norm["out"], norm["hits"], 1)
        assert need.any() and (case.startswith(("b", "d")) or not need.all())  # (b, d: every read falls back to the normal call)
    nar, num_hits, hits0 = out["nar"].copy(), out["num_hits"].copy(), hits[:, 0].copy()
    where = [(index_names[int(x["chrom_id"]) - 1], int(x["match_loci"]) + 1, chr(int(x["strand"]))) if x["chrom_id"] else None for x in hits0]
    if regions is not None and "-V" not in args:
        n_pr = priority_ref.filter_regions(regions, nar, num_hits, hits0)
        assert n_pr == meta["nar"].get("PR", 0)
    want = golden_reads(case)
    assert len(want) == len(names)
    mine = {nm: (where[i] if nar[i] == 1 else NAR_CODES[nar[i]]) for i, nm in enumerate(names)}
    assert mine == want
    for code in ("AA", "ML", "PR", "NL"):
        assert int((nar == NAR_CODES.index(code)).sum()) == meta["nar"].get(code, 0), code


def test_bed_interval_semantics():
    """the end column is exclusive: a feature `x 3000 3100` holds the loci 3000..3099; a span that abuts it misses it, one base of
    overlap at either end meets it (the reads of case f around the feature are placed accordingly by the test above)"""
    r = priority_ref.Regions("# c\ntrack name=t\nx\t3000\t3100\tf\t0\t.\nX 6000 6001\nnosuch 0 10\nx 5000 5000\nx 0 0\n", ["w", "x"])
    assert sorted(r.by_entry) == [2] and r.by_entry[2] == [(3000, 3099), (6000, 6000), (5000, 4999)]
    # a feature of no bases: met by a span that covers both 4999 and 5000
    assert r.in_any_feature(2, 4901, 5000) and not r.in_any_feature(2, 4900, 4999) and not r.in_any_feature(2, 5000, 5099)
    assert not r.in_any_feature(2, 2900, 2999) and r.in_any_feature(2, 2901, 3000)
    assert r.in_any_feature(2, 3099, 3198) and not r.in_any_feature(2, 3100, 3199)
    assert r.in_any_feature(2, 5950, 6049) and not r.in_any_feature(1, 3000, 3099) and not r.in_any_feature(3, 0, 5)
    from oracle_bindings import HIT_DTYPE
    h = np.zeros(40000, HIT_DTYPE)  # the array form of the test equals the literal one
    rng = np.random.default_rng(1)
    h["chrom_id"], h["match_loci"], h["match_len"] = rng.integers(0, 4, 40000), rng.integers(2800, 6200, 40000), rng.integers(1, 150, 40000)
    assert np.array_equal(r.mask(h), np.array([r.hit_in_feature(x) for x in h])) and 0 < r.mask(h).sum() < 20000
    ids, starts, ends = r.intervals()
    assert ids.tolist() == [2, 2, 2] and starts.tolist() == [3000, 6000, 5000] and ends.tolist() == [3099, 6000, 4999]
    assert priority_ref.locate_chrom(["ChrC", "chr1"], "chloroplast") == 0 and priority_ref.locate_chrom(["mitochondria"], "chrm") == 0
    with pytest.raises(ValueError):
        priority_ref.read_bed("x 5 4\n")


def test_case_f_has_the_edge_reads_on_both_sides():
    """around uniq:3000-3100, and around the feature of no bases uniq:5000-5000, which the reference keeps as 5000..4999: a span meets it
    when it covers 4999 and 5000"""
    sys.path.insert(0, GOLDEN)
    from make_golden_priority import EDGE_STARTS

    got = golden_reads("f")
    n_in = 0
    for k in range(2 * len(EDGE_STARTS)):
        v, s = got["edge%04d" % k], EDGE_STARTS[k // 2]
        inside = (s + 99 >= 3000 and s <= 3099) or (s <= 4999 and s + 99 >= 5000)
        assert (v == "PR") == (not inside), (k, s, v)
        if inside:
            assert v[:2] == ("uniq", s + 1)
            n_in += 1
    assert n_in == 2 * (6 + 3)  # starts 2901..3099 and 4901..4999


def test_b_r2_R5_draws_among_the_hits_the_unstable_compaction_leaves(oracle):
    """-r2 -R5 on the segment in three copies, two of them covered: the reference goes on with two instances and draws one.  Which two
    is the rule of KAligner.cpp:9732-9755 -- [P1, N, P2] leaves [P2, N] -- so the uncovered copy is drawn for some reads; every read
    of the golden lies on one of the hits the restatement keeps, and both kept hits are drawn."""
    O, h, index_names = oracle
    meta = CASES["b_r2_R5"]
    names, seqs = fasta("priority_tri.fa.xz")
    reads = [np.array([CODE[c] for c in s], np.uint8) for s in seqs]
    regions = priority_ref.Regions(open(os.path.join(GOLDEN, "priority_%s.bed" % meta["bed"])).read(), index_names)
    kw = dict(max_subs=2, pe_mode=2)
    norm = O.kalign_batch(h, reads, max_ml=5, **kw)
    wide = O.kalign_batch(h, reads, max_ml=5 + priority_ref.PRIORITY_EXACTS, **kw)
    out, hits, need = priority_ref.select(regions, wide["out"], wide["hits"], norm["out"], norm["hits"], 5, 2)
    want = golden_reads("b_r2_R5")
    loc = lambda x: (index_names[int(x["chrom_id"]) - 1], int(x["match_loci"]) + 1, chr(int(x["strand"])))  # noqa: E731
    drawn_slot, outsider_drawn = set(), 0
    for i, nm in enumerate(names):
        assert out[i]["nar"] == 1 and want[nm] != "ML", nm
        allowed = [loc(hits[i, q]) for q in range(int(out[i]["num_hits"]))]
        assert want[nm] in allowed, (nm, want[nm], allowed)
        if len(allowed) == 2:
            assert not need[i]
            drawn_slot.add(allowed.index(want[nm]))
            outsider_drawn += not regions.hit_in_feature(hits[i, allowed.index(want[nm])])
    assert drawn_slot == {0, 1} and outsider_drawn > 0
    assert (~need).sum() >= 150


# ---- k4align's argument rules (no device is touched before they are checked) ---------------------------------------------------------
def _run(args):
    return subprocess.run([K4ALIGN] + args, capture_output=True, text=True, timeout=60)


BASE = ["-i", "/nonexistent/reads.fa", "-I", "/nonexistent/x.sfx", "-o", "/nonexistent/o.sam"]
BED = os.path.join(GOLDEN, "priority_trusted.bed")


def test_a_missing_bed_file_exits_2():
    p = _run(BASE + ["--priorityregionfile", "/nonexistent/regions.bed"])
    assert p.returncode == 2 and "Unable to open high priority regions BED file '/nonexistent/regions.bed'" in p.stderr
    p = _run(BASE + ["--priorityregionfile=/nonexistent/regions.bed", "-V"])
    assert p.returncode == 2 and "Unable to open high priority regions BED file" in p.stderr


@pytest.mark.parametrize("extra", [["-r5", "-R8", "-X"], ["-r5", "-R8", "-N"], ["-M3", "--experimentid", "e", "--readsetid", "r"]])
def test_refused_combinations_exit_3(extra):
    p = _run(BASE + ["--priorityregionfile", BED] + extra)
    assert p.returncode == 3 and "not built" in p.stderr, p.stderr


def test_flags_take_no_value_and_B_is_still_the_chunk_size():
    # -V, --nofiltpriority: flags (the option behind them is read as an option); without a file they do nothing; -B 4: a number
    for flags in (["-V"], ["--nofiltpriority"], ["--nofiltpriority", "-V", "-B", "4"], ["-B4"]):
        p = _run(flags + BASE)
        assert p.returncode == 2 and "unable to load '/nonexistent/x.sfx'" in p.stderr and "usage" not in p.stderr.lower(), (flags, p.stderr)
    # the flag in front of the file option does not eat it
    p = _run(["--nofiltpriority", "--priorityregionfile", "/nonexistent/regions.bed"] + BASE)
    assert p.returncode == 2 and "high priority regions BED file" in p.stderr
    # a long name without its value is the usage error it was
    assert _run(BASE + ["--priorityregionfile"]).returncode == 1
