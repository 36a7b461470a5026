"""The crafted SNP scenarios (tests/snp_craft.py) hold what they are built for: checked on the oracle's four texts and on the plain
pile-up (tests/pba_ref.py), without a device.  tests/test_gpu_snp_crafted.py compares the device with the oracle on the same inputs;
what is asserted here keeps that comparison from passing on inputs that exercise nothing."""
import math

import pytest

import pba_ref
import snp_craft


@pytest.fixture(scope="module")
def run(oracle):
    """run(name, k): the materialised scenario, the oracle's files for its option set k and the plain pile-up, each made once"""
    files, piles = {}, {}

    def get(name, k=0):
        s = snp_craft.scenario(name)
        if (name, k) not in files:
            files[(name, k)] = snp_craft.oracle_files(oracle, s, k)
        if name not in piles:
            piles[name] = pba_ref.pileup(s["chroms"], s["piled"])
        return s, files[(name, k)], piles[name]

    return get


@pytest.mark.parametrize("name,k", snp_craft.CASES, ids=["%s-%d" % c for c in snp_craft.CASES])
def test_called_and_absent_loci_and_haplotype_lines(run, name, k):
    s, f, cnts = run(name, k)
    e, opts, names = s["expect"][k], s["opts"][k], s["names"]
    got = snp_craft.called(f["snp"])
    assert got == {names[c]: l for c, l in e["called"].items() if l}
    assert f["n_snps"] == sum(len(l) for l in e["called"].values())
    for c, loci in e["called"].items():  # every called locus passes the four tests on the plain pile-up too
        for l in loci:
            assert snp_craft.why_not(cnts[c], l, opts) is None, (c, l)
    for (c, l), why in e["absent"].items():
        assert l not in got.get(names[c], []), (c, l)
        assert snp_craft.why_not(cnts[c], l, opts) == (None if why == "cut" else why), (c, l, why)
    for key, text in (("di", f["disnp"]), ("tri", f["trisnp"])):
        want = sorted((names[c], t) for c, ts in e.get(key, {}).items() for t in ts)
        assert sorted((x[0], x[1]) for x in snp_craft.hap_lines(text)) == want
    spans = snp_craft.wig_spans(f["wig"])
    assert all(l > 0 for sp in spans.values() for l, _, _ in sp)  # the span that starts at locus 0 is lost ...
    if name != "skips":
        assert any(int(cnt[0, 0] + cnt[1, 0]) > 0 for cnt in cnts.values())  # ... and a sequence is covered there
    assert set(spans) <= {names[c] for c in cnts}


def test_windows_differ_across_the_clamping_edges(run):
    s, f, cnts = run("windows")
    rows = snp_craft.csv_rows(f["snp"])
    for c, a, b in s["expect"][0]["edges"]:
        ra, rb = rows[(s["names"][c], a)], rows[(s["names"][c], b)]
        assert ra[19] != rb[19], (c, a, b)  # TotWinBases
    assert 11 not in cnts and (cnts[10][:, 170:230] == 0).all()  # no read on m11; the N run counts nothing
    assert int(rows[("m10", 169)][19]) < 51 * 8 - 8 - 25 * 6  # the window of 169 holds 25 N loci
    assert snp_craft.why_not(cnts[0], 0, s["opts"][0]) == "noise" and int(cnts[0][1, 0]) == 8
    n_noise = sum(int(((cnt[1] == 1) & (cnt[0] >= 5)).sum()) for cnt in cnts.values())
    assert n_noise > 100  # single substituted reads between the SNPs


@pytest.mark.parametrize("k", [0, 1])
def test_thresholds_sit_on_their_equalities(run, k):
    s, f, cnts = run("thresholds", k)
    cnt, opts = cnts[0], s["opts"][k]
    tot = cnt[0].astype(int) + cnt[1].astype(int)
    assert tot[1550] == opts["min_snp_reads"] and tot[1750] == opts["min_snp_reads"] - 1 and cnt[1, 1750] == 4
    assert (cnt[1, 100], tot[100]) == (2, 8) and 2 / 8 == opts["snp_nonref_pcnt"] / 100.0
    assert (cnt[1, 1520], tot[1520]) == (1, 5)
    assert cnt[6, 40] == cnt[1, 40] == 8 and cnt[6, 300] == cnt[1, 300] == 8
    rows = snp_craft.csv_rows(f["snp"])
    for l in range(896, 906):
        assert rows[("m00", l)][18:21] == ["0.197500", "400", "79"]
    assert rows[("m00", 1550)][10:12] == ["5", "5"] and rows[("m00", 40)][13:18] == ["0", "0", "0", "0", "8"]
    spans = snp_craft.wig_spans(f["wig"])
    assert spans["m00"] == [(1500, 100, 5), (1700, 100, 4)]
    assert spans["m01"] == [(10, 590, 8)]  # closed by candidates that need not survive the cut
    if k == 0:
        assert rows[("m00", 100)][10:12] == ["8", "2"] and 0.0001 < float(rows[("m00", 100)][9]) < 0.05
    else:
        assert "m01" not in snp_craft.called(f["snp"])
        assert all(float(r[9]) == 0.0 for r in rows.values())


def test_haplotype_reads_end_where_they_should(run):
    s, f, cnts = run("haplotypes")
    e = s["expect"][0]
    di = {(x[0], x[1]): x[2:] for x in snp_craft.hap_lines(f["disnp"])}
    tri = {(x[0], x[1]): x[2:] for x in snp_craft.hap_lines(f["trisnp"])}
    # depth of each line: which reads count
    assert di[("m00", (300, 320))][0] == 12 + 2 + 2                  # + the reads that start at 300 / end at 320
    assert di[("m00", (600, 615))][0] == 18 + 3 + 2 and di[("m00", (615, 630))][0] == 18 + 3 + 2  # an N at the third / first locus
    assert tri[("m00", (600, 615, 630))][0] == 18                    # no read with an N
    assert all(tri[("m00", t)][::2] == (18, 3) for t in e["tri"][0][1:4])
    assert di[("m00", (1200, 1215))] == (14, 7, 2) and di[("m00", (1350, 1365))] == (65, 32, 3)
    assert di[("m00", (2700, 2720))][0] == 18 + 6 and di[("m00", (2720, 2740))][0] == 18 + 6 and tri[("m00", (2700, 2720, 2740))][0] == 18 + 4
    assert all(0 < x[1] < x[0] for x in list(di.values()) + list(tri.values()))  # both strands in every line
    line = [l for l in f["disnp"].splitlines() if ",1200," in l][0].split(",")
    assert sorted(int(x) for x in line[-16:])[-3:] == [0, 5, 5]      # AR x 4 printed as 0
    line = [l for l in f["trisnp"].splitlines() if ",910," in l and ",930," in l][0].split(",")
    assert sorted(int(x) for x in line[-64:])[-4:] == [0, 6, 6, 6]
    # the pairs without a line: why
    spans_both = lambda c, a, b: sum(1 for cc, st, bs in s["piled"] if cc == c and st <= a and st + len(bs) > b)  # noqa: E731
    assert spans_both(0, 1800, 1830) == s["opts"][0]["min_snp_reads"] - 1
    assert spans_both(0, 1500, 1515) == 10 and spans_both(0, 2400, 2459) == 12 and spans_both(2, 1500, 1801) == 12
    for c, pairs in e["no_di"].items():
        for p in pairs:
            assert (s["names"][c], p) not in di
    # max_sep: the ceiling of a mean that is no integer on m00, 300 under 400-base reads on m02
    lens = [len(bs) for c, _, bs in s["piled"] if c == 0]
    assert math.ceil(sum(lens) / len(lens)) == snp_craft.HAP_MAX_SEP == 2158 - 2100 and sum(lens) % len(lens)
    assert {len(bs) for c, _, bs in s["piled"] if c == 2} == {400}
    assert len(e["called"][3]) == 1 and len(e["called"][4]) == 2
    # trimmed reads: flagged, on both strands, their flanks full of mismatches that nothing may count
    trimmed = [a for a in s["alns"] if a[6] & snp_craft.EXT_CHIMERIC]
    assert len(trimmed) == 10 and {a[3] for a in trimmed} == {False, True} and all(a[4] or a[5] for a in trimmed)
    assert int(cnts[0][1, 2681:2700].sum()) == 0


def test_pe_form_is_the_same_run(run):
    s, f, _ = run("pe_form")
    _, g, _ = run("haplotypes")
    assert f == g and len(s["pe_reads"]) == len(s["pe_recs"]) and len(s["pe_recs"]) % 2 == 0
    assert (s["pe_recs"]["nar"] != 1).sum() == len(s["pe_recs"]) - len(s["reads"])


def test_skipped_alignments_leave_nothing(run):
    s, f, cnts = run("skips")
    assert sorted(cnts) == [3]
    assert set(snp_craft.wig_spans(f["wig"])) == {"m03"}
    by_seq = {c: [a for a in s["alns"] if a[0] == c] for c in range(4)}
    assert all(a[6] & (snp_craft.EXT_INDEL | snp_craft.EXT_SPLICE) and a[7] == 1 for a in by_seq[0]) and len(by_seq[0]) == 10
    for a in by_seq[1]:
        lead, trail = (a[5], a[4]) if a[3] else (a[4], a[5])
        assert a[1] + lead + (len(a[2]) - lead - trail) == len(s["chroms"][1]) + 1 and a[7] == 1
    assert sorted(a[7] for a in by_seq[2]) == [0, 2, 3, 4, 5, 6, 7, 8, 9, 10]


def test_coverage_forms_and_wig_bookkeeping(run):
    s, f, cnts = run("coverage")
    depth = lambda c: int((cnts[c][0] + cnts[c][1]).max())  # noqa: E731
    assert [depth(c) for c in range(3)] == list(snp_craft.COV_DEEP) and depth(0) < 256 <= depth(1) < 65536 <= depth(2)
    rows = snp_craft.csv_rows(f["snp"])
    assert rows[("m02", 115)][10:12] == ["70000", "7000"] and int(1000.0 / 70000 * 7000) in (99, 100)  # Binomial's n > 5000
    spans = snp_craft.wig_spans(f["wig"])
    assert [spans["m%02d" % c] for c in range(3)] == [[(100, 30, n)] for n in snp_craft.COV_DEEP]
    cov3 = cnts[3][0] + cnts[3][1]
    assert len(cov3) > 200000 and (cov3 == 6).all()
    assert spans["m03"] == [(100000, 100000, 6), (200000, snp_craft.COV_LONG - 200000, 6)]
    closed = []
    for c in range(4, 4 + snp_craft.COV_SHORT):
        half = len(s["chroms"][c]) // 2
        sp = spans["m%02d" % c]
        assert sp[0] == (3, half - 3, 6) and sp[1:] in ([], [(half, len(s["chroms"][c]) - half, 9)])
        closed.append(len(sp) == 2)
    assert closed == [True, False] * (snp_craft.COV_SHORT // 2) and len(cnts) == 20 > 12 + 2


def test_vcf_keeps_the_strings_of_the_snp_before(run):
    s, f, _ = run("vcf")
    recs = {int(r.split("\t")[1]): r.split("\t") for r in f["snp"].splitlines() if r.startswith("m00")}
    first = f["snp"].splitlines()[0].split("\t")
    assert first[:3] == ["m00", "41", "SNP1"] and first[4] == "" and first[7] == "AF=;DP=8"
    assert recs[201][4] in "ACGT" and len(recs[201][4]) == 1 and recs[201][7] == "AF=1.0000;DP=8"
    assert recs[301][4] == recs[201][4] and recs[301][7] == recs[201][7]
