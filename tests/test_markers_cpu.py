"""kalign's SNP centroids (-7) and marker sequences (-K) without a GPU: the Python restatement (tests/markers_ref.py) against the files
`ngskit4b kalign` wrote (tests/golden/cent_* / mk_*, make_golden_markers.py), the library's host rule (k4_marker_classify_host -- the
same function the kernel runs) against the restatement on an exact-threshold grid, k4align's option rules, and the new ABI symbols."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import markers_ref
import pba_ref
import samutil
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MARKER_CASES = json.load(open(os.path.join(GOLDEN, "markers_cases.json")))
K4ALIGN = os.path.join(ROOT, "kit4b_amd", "k4align")


def marker_args(args):
    """the SNP / marker keywords of SfxIndex.snp_files from a kalign argument list"""
    kw = {}
    for i, a in enumerate(args):
        if a.startswith("-p"):
            kw["min_snp_reads"] = int(a[2:])
        elif a.startswith("-P"):
            kw["qvalue"] = float(a[2:])
        elif a.startswith("-1"):
            kw["snp_nonref_pcnt"] = float(a[2:])
        elif a.startswith("-K"):
            kw["marker_len"] = int(a[2:])
        elif a == "--markerpolythres":
            kw["marker_poly_thres"] = float(args[i + 1])
        elif a == "-7":
            kw["centroids"] = True
    return kw


def golden_text(name):
    path = os.path.join(GOLDEN, name)
    return lzma.open(path + ".xz").read().decode() if os.path.exists(path + ".xz") else open(path).read()


def snp_file_of(case):
    meta = MARKER_CASES[case]
    return golden_text((meta["reads"] if case.startswith("cent_") else case) + meta["ext"])


@pytest.fixture(scope="module")
def genome():
    return synth.golden_genome()


@pytest.fixture(scope="module")
def piled(genome):
    """{reads: per-chromosome counts} from the reference's SAM of each read set the cases use; once"""
    names, chroms = genome
    out = {}
    for reads in sorted({m["reads"] for m in MARKER_CASES.values()}):
        _, recs = samutil.read_sam_xz(os.path.join(GOLDEN, reads + ".sam.xz"))
        out[reads] = pba_ref.pileup(chroms, pba_ref.sam_alignments(recs, names))
    return out


@pytest.fixture(scope="module")
def restated(genome, piled):
    names, chroms = genome
    out = {}
    for case, meta in MARKER_CASES.items():
        kw = marker_args(meta["args"])
        out[case] = markers_ref.run(names, chroms, piled[meta["reads"]], kw.get("min_snp_reads", 5), kw.get("snp_nonref_pcnt", 25.0), kw.get("marker_len", 0),
                                    kw.get("marker_poly_thres", markers_ref.DFLT_POLY_THRES))
    return out


@pytest.mark.parametrize("case", sorted(MARKER_CASES))
def test_restatement_equals_the_reference(genome, piled, restated, case):
    names, chroms = genome
    meta, r = MARKER_CASES[case], restated[case]
    called, cols = markers_ref.called_loci(snp_file_of(case), names)
    assert len(called) == meta["snps"]
    for c, l in called:  # the called loci are among those the restatement lets through to the p-value
        assert l in set(r["survivors"][c]), (c, l)
    if "-7" in meta["args"]:
        text = markers_ref.centroid_text(r["insts"], chroms, piled[meta["reads"]], called)
        assert text == golden_text(case + ".centroids.csv")
        assert int(r["insts"].sum()) == meta["insts"] > meta["cent_snps"] > 0
    if "markers" in meta:
        assert r["markers"] == golden_text(case + ".markers")
        assert r["n_markers"] == meta["markers"]
        for key, ids in cols.items():  # MarkerID and NumPolymorphicSites, the CSV's last two columns
            assert r["ids"][key] == ids
    else:
        assert all(ids == (0, 0) for ids in cols.values())


def test_goldens_exercise_the_gate(restated):
    """the marker cases reject candidates for every reason but the chromosome's ends, and at least one marker has a polymorphic site"""
    why = {}
    for case, r in restated.items():
        for k, n in r["rejects"].items():
            why[k] = why.get(k, 0) + n
    assert {"proportion", "coverage", "allele"} <= set(why), why
    assert any(poly > 0 for r in restated.values() for _, poly in r["ids"].values())
    assert len(restated["mk_se_hap_K25"]["ids"]) != len(restated["mk_se_hap_K26_vcf"]["ids"])  # an even length moves the 3' flank


def test_window_sums_follow_the_reference_loop(piled):
    """the prefix-sum form of the background window against the reference's own sliding loop, on a golden chromosome and on short ones"""
    rng = np.random.default_rng(5)
    cnt7 = piled["snp_se"][2]
    seqs = [(cnt7[0], cnt7[1])] + [(rng.integers(0, 9, n), rng.integers(0, 3, n)) for n in (1, 25, 26, 50, 51, 52, 53, 77, 103)]
    for n_ref, n_non in seqs:
        n_ref, n_non = np.asarray(n_ref, np.int64), np.asarray(n_non, np.int64)
        clen, win = len(n_ref), 51
        l = np.arange(clen)
        lo = np.where(l <= 25, 0, np.where(l + 25 < clen, l - 25, clen - win)) if clen > win else np.zeros(clen, np.int64)
        hi = np.minimum(lo + win, clen)
        p_ref, p_non = np.concatenate([[0], np.cumsum(n_ref)]), np.concatenate([[0], np.cumsum(n_non)])
        want = markers_ref.sliding_window_sums(n_ref, n_non)
        assert [(int(a), int(b)) for a, b in zip(p_ref[hi] - p_ref[lo], p_non[hi] - p_non[lo])] == want


# ---- the per-locus rule on the host: the proportions that land exactly on a threshold ----------------------------------------------
def host_rule(cols, min_snp_reads, thres):
    import kit4b_amd

    cnt7 = np.array([[x[0] for x in cols], [x[1] for x in cols]] + [[x[2][b] for x in cols] for b in range(5)], np.uint32)
    base, poly = kit4b_amd.marker_classify_host(cnt7, np.array([x[3] for x in cols], np.uint8), min_snp_reads, thres)
    return [("coverage" if b == 0xff else "allele" if b == 0xfe else int(b), bool(p)) for b, p in zip(base, poly)]


def test_host_rule_on_the_exact_grid():
    """every coverage 1..40, every non-reference count, one or two alleles, thresholds whose 1 - t is and is not exact in binary:
    what IEEE doubles decide at 1/10, 9/10, 1/2, t and 1 - t is what the restatement's Python floats decide"""
    for thres in (0.0, 0.1, 0.2, 0.25, 0.3, 1.0 / 3.0, 0.4, 0.5):
        for min_reads in (1, 5):
            cols = []
            for tot in range(1, 41):
                for non in range(tot + 1):
                    ref = tot % 4
                    a1 = (ref + 1) % 4
                    cols.append((tot - non, non, [non if b == a1 else 0 for b in range(5)], ref))  # one allele
                    if non >= 2:  # two alleles: the smaller one comes first in A, C, G, T order
                        a, b2 = sorted([(ref + 1) % 4, (ref + 2) % 4])
                        cols.append((tot - non, non, [1 if b == a else non - 1 if b == b2 else 0 for b in range(5)], ref))
                        cols.append((tot - non, non, [0, 0, 0, 0, non], ref))  # all N
            want = [markers_ref.marker_locus(c[0], c[1], c[2], c[3], min_reads, thres) for c in cols]
            assert host_rule(cols, min_reads, thres) == want, (thres, min_reads)


def test_host_rule_at_each_threshold():
    A, C, G, T, N = range(5)
    t = 0.2
    cases = [
        # (n_ref, n_non, [A, C, G, T, N], ref, min reads) -> (base | rejection, polymorphic)
        ((8, 2, [0, 2, 0, 0, 0], A, 5), (A, True)),          # 2/10 == t: the reference base; 0.2 > 0.1: polymorphic
        ((9, 1, [0, 1, 0, 0, 0], A, 5), (A, False)),         # 1/10 is not > 0.1
        ((18, 2, [0, 2, 0, 0, 0], G, 5), (G, False)),        # 2/20 == 0.1: not polymorphic
        ((17, 3, [0, 3, 0, 0, 0], G, 5), (G, True)),
        ((2, 8, [0, 8, 0, 0, 0], A, 5), (C, True)),          # 8/10 == 1 - t: accepted, 0.8 < 0.9: polymorphic
        ((1, 9, [0, 9, 0, 0, 0], A, 5), (C, False)),         # 9/10 is not < 0.9
        ((3, 7, [0, 7, 0, 0, 0], A, 5), ("allele", False)),  # 0.7 < 1 - t
        ((5, 5, [0, 5, 0, 0, 0], A, 5), ("allele", False)),  # 0.5: above t, below 1 - t
        ((5, 0, [0, 0, 0, 0, 0], T, 5), (T, False)),         # coverage exactly MinSNPreads
        ((4, 0, [0, 0, 0, 0, 0], T, 5), ("coverage", False)),  # one below
        ((0, 4, [0, 4, 0, 0, 0], T, 5), ("coverage", False)),
        ((0, 10, [0, 0, 0, 0, 10], A, 5), (N, False)),       # an N majority gives N
        ((0, 10, [0, 1, 0, 9, 0], A, 5), (T, False)),        # the second allele: C is > 0 but below 1 - t
        ((0, 0, [0, 0, 0, 0, 0], A, 1), ("coverage", False)),
    ]
    cols = [c for c, _ in cases]
    for min_reads in {c[4] for c in cols}:
        sel = [k for k, c in enumerate(cols) if c[4] == min_reads]
        got = host_rule([cols[k] for k in sel], min_reads, t)
        assert got == [cases[k][1] for k in sel]
        assert got == [markers_ref.marker_locus(*cols[k][:4], min_reads, t) for k in sel]
    # with t = 0.5 both branches meet: 5/10 takes the reference base, 6/10 the allele; first-of-five: equal counts give the lower base
    assert host_rule([(5, 5, [0, 5, 0, 0, 0], A, 5), (4, 6, [0, 0, 6, 0, 0], A, 5), (0, 10, [0, 0, 5, 5, 0], A, 5)], 5, 0.5) == [(A, True), (G, True), (G, True)]


def test_new_abi_symbols_are_declared():
    import ctypes as C

    import kit4b_amd

    assert {"k4_snp_run2_dev", "k4_marker_classify_host"} <= set(kit4b_amd.ABI_SYMBOLS)
    L = kit4b_amd.lib()
    assert len(L.k4_snp_run2_dev.argtypes) == 17 and len(L.k4_marker_classify_host.argtypes) == 8
    assert C.sizeof(kit4b_amd.SnpOpts) == 16 and C.sizeof(kit4b_amd.SnpFiles2) == C.sizeof(kit4b_amd.SnpFiles) + 40 == 112
    import inspect

    sig = inspect.signature(kit4b_amd.SfxIndex.snp_files).parameters
    assert sig["marker_len"].default == 0 and sig["marker_poly_thres"].default is None and sig["centroids"].default is False
    hdr = open(os.path.join(ROOT, "include", "k4sfx.h")).read()  # the four earlier entry points keep their declarations
    for s in ("k4_snp_csv_dev", "k4_snp_vcf_dev", "k4_snp_files_dev", "k4_snp_run_dev"):
        assert hdr.count("int %s(" % s) == 1


# ---- k4align: the rules are decided before the index is opened, so they run without a GPU ------------------------------------------
@pytest.fixture(scope="module")
def base(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("marker_opts")
    fa = tmp / "r.fa"
    fa.write_text(">r1\n" + "ACGT" * 25 + "\n")
    return [K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-i", str(fa), "-o", str(tmp / "o.sam")], tmp


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra", [["-K24"], ["-K", "501"], ["-K-5"], ["--markerlen", "24"], ["--markerlen=501"]])
def test_marker_length_range(base, extra):
    cmd, _ = base
    p = run(cmd + ["-p5"] + extra)
    assert p.returncode == 1 and "must be in range 25 to 500" in p.stderr, p.stderr


@pytest.mark.parametrize("extra", [["--markerpolythres", "0.51"], ["--markerpolythres=-0.1"]])
def test_marker_threshold_range(base, extra):
    cmd, _ = base
    p = run(cmd + ["-p5", "-K25"] + extra)
    assert p.returncode == 1 and "must be in range 0.0 to 0.5" in p.stderr, p.stderr


@pytest.mark.parametrize("extra", [["-K25"], ["-7", "c.csv"], ["--snpcentroid", "c.csv"], ["--markerlen", "30"]])
def test_markers_and_centroids_need_snp_calling(base, extra):
    cmd, tmp = base
    p = run(cmd + extra)
    assert p.returncode == 1 and "SNP calling" in p.stderr, p.stderr
    assert not os.path.exists(tmp / "c.csv")


@pytest.mark.parametrize("extra", [["-K25"], ["-7", "c.csv"], ["--snpcentroid=c.csv"], ["--markerlen", "30"], ["--markerpolythres", "0.2"]])
def test_genpba_has_neither(base, extra):
    cmd, tmp = base
    p = run(cmd[:-2] + ["-o", str(tmp / "o.pba"), "-M3", "--experimentid", "e", "--readsetid", "r"] + extra)
    assert p.returncode == 1 and "-M3" in p.stderr, p.stderr


def test_they_inherit_the_refusals_of_snp_calling(base):
    cmd, _ = base
    p = run(cmd + ["-p5", "-K25", "-b", "1"])
    assert p.returncode == 3
    p = run(cmd + ["-p5", "-7", "c.csv", "-b", "1"])
    assert p.returncode == 3
    p = run(cmd + ["-p5", "-K25", "-r5", "-R4"])
    assert p.returncode == 1 and "multiloci" in p.stderr
    p = run(cmd + ["-p5", "-K0", "-b", "1"])  # -K0: no markers, the plain SNP run's rules
    assert p.returncode == 3
