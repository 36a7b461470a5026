"""genpba's packed base alleles without a GPU: the Python restatement (tests/pba_ref.py) against the files `ngskit4b genpba` wrote
(tests/golden/pba_*.pba.xz / .covsegs.wig.xz, make_golden_pba.py), the library's host classifier (k4_pba_classify_host -- the same
function the kernel runs) against both, and k4align's option rules for `-M3`."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import pba_ref
import samutil
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PBA_CASES = json.load(open(os.path.join(GOLDEN, "pba_cases.json")))
K4ALIGN = os.path.join(ROOT, "kit4b_amd", "k4align")


@pytest.fixture(scope="module")
def genome():
    return synth.golden_genome()


@pytest.fixture(scope="module")
def restated(genome):
    """per case: (pba bytes, wig text, number of records, {chromosome: (counts, bytes, coverage)}) from the reference's SAM; once"""
    names, chroms = genome
    out = {}
    for case, meta in PBA_CASES.items():
        _, recs = samutil.read_sam_xz(os.path.join(GOLDEN, meta["sam"] + ".sam.xz"))
        out[case] = pba_ref.pba_files(names, chroms, pba_ref.sam_alignments(recs, names), meta["clean_ids"][0], "g1", meta["clean_ids"][1])
    return out


def golden_files(case):
    return (lzma.open(os.path.join(GOLDEN, case + ".pba.xz")).read(), lzma.open(os.path.join(GOLDEN, case + ".covsegs.wig.xz")).read().decode())


@pytest.mark.parametrize("case", sorted(PBA_CASES))
def test_restatement_equals_the_reference(restated, case):
    blob, wig = golden_files(case)
    got_blob, got_wig, n_chroms, _ = restated[case]
    assert got_blob == blob and len(blob) == PBA_CASES[case]["pba_bytes"]
    assert got_wig == wig and not wig.startswith("track")
    assert n_chroms == PBA_CASES[case]["n_chroms"] == len(pba_ref.parse_pba(blob)[1])


def test_goldens_hold_every_score_in_both_coverage_classes(restated):
    hist = np.zeros((2, 4), np.int64)
    for _, _, _, per in restated.values():
        for _, pb, cov in per.values():
            for sh in (6, 4, 2, 0):
                s = (pb >> sh) & 3
                hist[0] += np.bincount(s[(cov > 0) & (cov < 5)], minlength=4)
                hist[1] += np.bincount(s[cov >= 5], minlength=4)
    assert (hist[1] > 0).all() and (hist[0][:3] > 0).all() and hist[0][3] == 0


@pytest.mark.parametrize("case", sorted(PBA_CASES))
def test_host_classifier_on_the_golden_counts(genome, restated, case):
    import kit4b_amd

    _, chroms = genome
    by_name = dict(pba_ref.parse_pba(golden_files(case)[0])[1])
    per = restated[case][3]
    assert len(per) == len(by_name)
    for c, (cnt7, _, cov) in per.items():
        pba, got_cov = kit4b_amd.pba_classify_host(cnt7, chroms[c])
        assert np.array_equal(pba, by_name["chr%d" % (c + 1)])
        assert np.array_equal(got_cov, cov)


def test_host_classifier_on_the_exact_grid():
    """every coverage 1..40, every allele count 0..coverage, the allele being the target's base or not: the proportions that land
    exactly on a threshold (4/20, 7/20, 15/20, 3/4, 1/5, ...) are decided as IEEE doubles decide them"""
    import kit4b_amd

    cols, want = [], []
    for cov in range(1, 41):
        for c in range(cov + 1):
            for allele in range(4):
                other = (allele + 1) % 4
                # the allele is the target's base: c reference reads, the rest on another base; an N read on top that coverage leaves out
                cols.append((c, cov - c + 1, [cov - c if b == other else 0 for b in range(4)] + [1], allele))
                # the allele is not the target's base (which is `other`): c non-reference reads of it
                cols.append((cov - c, c, [c if b == allele else 0 for b in range(4)] + [0], other))
    for n_ref, n_non, by_base, ref in cols:
        want.append(pba_ref.classify_locus(n_ref, n_non, by_base, ref))
    cnt7 = np.array([[x[0] for x in cols], [x[1] for x in cols]] + [[x[2][b] for x in cols] for b in range(5)], np.uint32)
    ref = np.array([x[3] for x in cols], np.uint8)
    pba, cov = kit4b_amd.pba_classify_host(cnt7, ref)
    assert pba.tolist() == [w[0] for w in want] and cov.tolist() == [w[1] for w in want]
    assert np.array_equal(pba, pba_ref.classify(cnt7, ref))  # (the vectorised form the file restatement uses)
    # the rounded quotient against the rounded literal, not the exact rational: these are what an integer restatement could move
    exact = [(7, 20, 2), (4, 20, 1), (15, 20, 3), (6, 8, 3), (1, 5, 1), (2, 5, 2), (3, 4, 2), (1, 3, 1), (6, 20, 1), (14, 20, 2), (3, 20, 0)]
    cnt7 = np.zeros((7, len(exact)), np.uint32)
    for k, (c, n, _) in enumerate(exact):  # c reads show the target's A, the others a C
        cnt7[0, k], cnt7[1, k], cnt7[3, k] = c, n - c, n - c
    pba, cov = kit4b_amd.pba_classify_host(cnt7, np.zeros(len(exact), np.uint8))
    assert (pba >> 6).tolist() == [s for _, _, s in exact] and cov.tolist() == [n for _, n, _ in exact]


def test_host_classifier_edges():
    import kit4b_amd

    # no coverage; N reads only (coverage 0, byte 0); a target base that is no allele (never reached by the pile-up: all non-reference)
    cnt7 = np.array([[0, 0, 0], [0, 3, 6], [0, 0, 6], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 3, 0]], np.uint32)
    pba, cov = kit4b_amd.pba_classify_host(cnt7, np.array([0, 1, 4], np.uint8))
    assert pba.tolist() == [0, 0, 0xC0] and cov.tolist() == [0, 0, 6]
    pba, cov = kit4b_amd.pba_classify_host(np.zeros((7, 0), np.uint32), np.zeros(0, np.uint8))
    assert len(pba) == 0 and len(cov) == 0


def test_new_abi_symbols_are_declared():
    import kit4b_amd

    assert {"k4_pba_run_dev", "k4_pba_classify_host"} <= set(kit4b_amd.ABI_SYMBOLS)
    L = kit4b_amd.lib()
    assert len(L.k4_pba_run_dev.argtypes) == 14 and len(L.k4_pba_classify_host.argtypes) == 6
    assert hasattr(kit4b_amd.SfxIndex, "pba")


# ---- k4align -M3: the rules are decided before the index is opened, so they run without a GPU -------------------------------------
@pytest.fixture(scope="module")
def base(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pba_opts")
    fa = tmp / "r.fa"
    fa.write_text(">r1\n" + "ACGT" * 25 + "\n")
    return [K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-i", str(fa)], tmp


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=60)


IDS = ["--experimentid", "e1", "--readsetid", "r1"]


@pytest.mark.parametrize("extra", [["-a5"], ["-A", "500"], ["-O", "st.csv"], ["-j", "none.fa"], ["-J", "multi.fa"], ["-8", "sp.csv"], ["-9", "3"],
                                   ["--siteprefs", "sp.csv"], ["--siteprefsofs=3"], ["-5", "lc.csv"], ["--lociconstraints", "lc.csv"], ["-p5"],
                                   ["-P0.05"], ["-1", "10.0"], ["-N"], ["-S", "snps.csv"]])
def test_options_genpba_does_not_have_exit_1(base, extra):
    cmd, tmp = base
    p = run(cmd + ["-o", str(tmp / "o.pba"), "-M3"] + IDS + extra)
    assert p.returncode == 1 and "-M3" in p.stderr, p.stderr
    assert not os.path.exists(tmp / "o.pba") and not os.path.exists(tmp / "o.covsegs.wig")


@pytest.mark.parametrize("ids", [[], ["--experimentid", "e1"], ["--readsetid", "r1"], ["--experimentid", " \"' ", "--readsetid", "r1"],
                                 ["--experimentid=e1", "--readsetid", "  "]])
def test_both_ids_are_required(base, ids):
    cmd, tmp = base
    p = run(cmd + ["-o", str(tmp / "o.pba"), "-M3"] + ids)
    assert p.returncode == 1 and ("identifier" in p.stderr or "--experimentid" in p.stderr), p.stderr


@pytest.mark.parametrize("extra", [["-b", "1"], ["-S", "0/2"], ["-G", "0,1"], ["-Z"], ["-r5", "-R4"], ["-o", "x.BAM"]])
def test_combinations_that_are_not_built_exit_3(base, extra):
    cmd, tmp = base
    p = run(cmd + ["-o", str(tmp / "o.pba"), "-M3"] + IDS + extra)
    assert p.returncode == 3 and "not built" in p.stderr, p.stderr


def test_other_formats_keep_their_rules(base):
    cmd, tmp = base
    p = run(cmd + ["-o", str(tmp / "o.sam"), "-M2"])
    assert p.returncode == 3 and "not built" in p.stderr
    p = run(cmd + ["-o", str(tmp / "o.sam"), "-M7"])
    assert p.returncode == 1 and "range 0..3" in p.stderr
    p = run(cmd + ["-o", str(tmp / "o.sam")] + IDS)  # the ids belong to -M3
    assert p.returncode == 1 and "-M3" in p.stderr
