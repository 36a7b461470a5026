"""kalign's start-site octamer preferences (`-8`, `-9`) without a GPU: the restatement in tests/siteprefs_ref.py reproduces, byte for
byte, the file the reference binary wrote (tests/golden/make_golden_siteprefs.py) from the reference's own SAM of the same run; the
tie rule of the scale step does not show in any golden; the 32-bit arithmetic of the locus; and the argument rules of `k4align -8`."""
import json
import lzma
import os
import subprocess
import sys

import numpy as np
import pytest

import siteprefs_ref as R
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
K4ALIGN = os.path.join(os.path.dirname(HERE), "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "siteprefs_cases.json")))
_genomes = {}


def genome_of(index):
    if index not in _genomes:
        if index == "g1":
            _genomes[index] = synth.golden_genome()
        elif index == "g2":
            _genomes[index] = synth.cluster_genome()[:2]
        else:
            sys.path.insert(0, GOLDEN)
            from make_golden_ext import genome

            _genomes[index] = genome()[:2]
    return _genomes[index]


def golden(case, ext):
    return lzma.open(os.path.join(GOLDEN, "siteprefs_%s.%s.xz" % (case, ext)), "rt").read()


def ofs_of(args):
    return int(args[args.index("-9") + 1]) if "-9" in args else -4


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_reproduces_the_reference_file(case):
    names, chroms = genome_of(CASES[case]["index"])
    recs = R.records_of_sam(golden(case, "sam"), names)
    assert len(recs) == CASES[case]["nar"]["AA"]
    occ, sites = R.walk(recs, chroms, ofs_of(CASES[case]["args"]))  # (raises on a read in the undefined range: none in a golden)
    want = golden(case, "csv")
    assert R.text(occ, sites, len(recs)) == want
    # the stable-sort rule is not what makes this pass: the reversed tie order gives the same bytes
    assert R.text(occ, sites, len(recs), reverse_ties=True) == want
    assert library_text(occ, sites, len(recs)) == want  # the library's host finish (k4_write_site_prefs) over the same counts
    if recs:
        assert all(R.boundary_untied(occ[s], sites[s]) for s in (0, 1))
        assert want.count("\n") == 1 + 2 * 0xFFFF and "tttttttt" not in want and ',"tttttttg",' in want
        # the numpy form used on millions of records counts the same
        col = lambda k: [r[k] for r in recs]  # noqa: E731
        occ2, sites2 = R.walk_arrays(col("chrom"), col("loci"), col("mlen"), [r["strand"] == "-" for r in recs], col("segs"), chroms,
                                     ofs_of(CASES[case]["args"]))
        assert np.array_equal(occ, occ2) and np.array_equal(sites, sites2)
    else:
        assert want == ""


def library_text(occ, sites, n_accepted):
    """k4_write_site_prefs over given counts: no device is needed for the scale step and the text"""
    import ctypes as C
    import tempfile

    import kit4b_amd

    L = kit4b_amd.lib()
    blk = np.ascontiguousarray(np.concatenate([occ[0], occ[1], sites[0], sites[1]]).astype(np.uint32))
    sp = kit4b_amd.SitePrefs()
    u32p = C.POINTER(C.c_uint32)
    base = blk.ctypes.data
    for k in (0, 1):
        sp.num_occs[k] = C.cast(base + 4 * 65536 * k, u32p)
        sp.num_sites[k] = C.cast(base + 4 * 65536 * (2 + k), u32p)
    sp.n_accepted, sp.n_counted, sp.block = n_accepted, int(occ.sum()), base
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "s.csv")
        assert L.k4_write_site_prefs(C.byref(sp), path.encode()) == 0
        return open(path).read()


def test_library_tie_rule_equals_the_restatement():
    occ, sites = np.zeros((2, R.N_OCT), np.int64), np.zeros((2, R.N_OCT), np.int64)
    occ[0, :100], sites[0, :100] = 2, 1
    occ[0, :10] = 6
    occ[1, 7], sites[1, 7] = 5, 2           # fewer than 64 non-zero octamers: the highest zero-count ones get 1.000
    occ[1, 65535], sites[1, 65535] = 9, 1   # (tttttttt is counted and scaled, and not written)
    assert library_text(occ, sites, 3) == R.text(occ, sites, 3)
    assert library_text(occ, sites, 0) == ""


def test_locus_arithmetic():
    L = 1000
    # s = -9: wraps to a huge unsigned value and is "clamped" to the octamer that ends one base in front of the sequence's end
    assert R.hit_loci(91, 100, "+", -100, L) == (L - 9, True)
    assert R.hit_loci(0, 100, "+", -100, L) == (L - 9, True)
    # s = -8 .. -1: HitLoci + 8 wraps below the length, GetSeq returns nothing
    assert R.hit_loci(92, 100, "+", -100, L) == (0xFFFFFFF8, False)
    assert R.hit_loci(3, 100, "+", -4, L) == (0xFFFFFFFF, False)
    assert R.hit_loci(4, 100, "+", -4, L) == (0, True)
    # an octamer that would end on the last base is moved one base to the left; one base earlier it stays
    assert R.hit_loci(L - 8, 100, "+", 0, L) == (L - 9, True)
    assert R.hit_loci(L - 9, 100, "+", 0, L) == (L - 9, True)
    assert R.hit_loci(L - 10, 100, "+", 0, L) == (L - 10, True)
    # Crick: MatchLoci + MatchLen - 1 - ofs - 7
    assert R.hit_loci(500, 100, "-", -4, L) == (596, True)
    assert R.hit_loci(L - 100, 100, "-", -4, L) == (L - 9, True)


def test_walk_quirks():
    rng = np.random.default_rng(5)
    g = [rng.integers(0, 4, 400).astype(np.uint8), rng.integers(0, 4, 400).astype(np.uint8)]
    g[0][200:204] = 4
    rec = lambda chrom, loci, strand="+", mlen=100, segs=False: dict(chrom=chrom, loci=loci, mlen=mlen, strand=strand, segs=segs)  # noqa: E731
    with pytest.raises(R.Undefined):
        R.walk([rec(1, 2)], g, -4)
    occ, sites = R.walk([rec(1, 2)], g, -4, skip_undefined=True)
    assert occ.sum() == 0
    # NumSites counts runs along the walk, for both strands together: + at 50, - ending there, + at 50 again -> the + site twice
    walk = [rec(1, 54), rec(1, 54, "-", mlen=60), rec(1, 54, mlen=101)]
    occ, sites = R.walk(walk, g, -4)
    assert occ[0].sum() == 2 and sites[0].sum() == 2 and occ[1].sum() == 1 and sites[1].sum() == 1
    # a read over N and a two-segment read are transparent: the two reads at 54 stay one site
    walk = [rec(1, 54), rec(1, 200), rec(1, 300, segs=True), rec(1, 54)]
    occ, sites = R.walk(walk, g, -4)
    assert occ[0].sum() == 2 and sites[0].sum() == 1
    # the same locus as last of one sequence and first of the next is two sites
    occ, sites = R.walk([rec(1, 54), rec(2, 54)], g, -4)
    assert sites[0].sum() == 2
    # the octamer: the eight bases from loci + ofs, first base most significant; Crick reverse complemented
    occ, _ = R.walk([rec(1, 54)], g, -4)
    assert occ[0, int("".join(str(b) for b in g[0][50:58]), 4)] == 1
    occ, _ = R.walk([rec(1, 0, "-", mlen=60)], g, -4)
    assert occ[1, int("".join(str(3 - b) for b in g[0][56:64][::-1]), 4)] == 1


def test_tie_rule_of_the_scale_step():
    occ, sites = np.zeros(R.N_OCT, np.int64), np.zeros(R.N_OCT, np.int64)
    occ[:100], sites[:100] = 2, 1      # a hundred octamers tie at 2.0: the stable sort puts the HIGHER octamers into the top 64
    rel = R.scale(occ, sites)
    assert rel[99] == 1.0 and rel[36] == 1.0 and rel[35] == 1.0 and rel[0] == 1.0  # (all equal the top mean: 2 / 2)
    occ[:10] = 6                        # ten at 6.0, ninety at 2.0: mean of the top 64 = (10 * 6 + 54 * 2) / 64
    rel = R.scale(occ, sites)
    top = (10 * 6 + 54 * 2) / 64
    assert rel[5] == 1.0 and rel[99] == 1.0 and rel[46] == 1.0 and rel[45] == 2 / top and rel[10] == 2 / top
    assert R.scale(occ, sites, reverse_ties=True)[10] == 1.0 and not R.boundary_untied(occ, sites)
    occ[200], sites[200] = 1, 50000     # the floor
    assert R.scale(occ, sites)[200] == 0.0001


# ---- the argument rules of k4align (no device is touched before they are checked) ---------------------------------------------------
def _run(*args):
    base = [K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-o", "/dev/null", "-i", os.path.join(GOLDEN, "names.fa")]
    return subprocess.run(base + list(args), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args", [["-9", "101"], ["-9", "-101"], ["--siteprefsofs=-101"], ["--siteprefsofs", "200"]])
def test_offset_out_of_range(tmp_path, args):
    p = _run("-8", str(tmp_path / "s.csv"), *args)
    assert p.returncode == 1 and "must be in range -100..100" in p.stderr
    assert not os.path.exists(tmp_path / "s.csv")


@pytest.mark.parametrize("args", [["-r5", "-R8"], ["-b", "1"], ["-S", "0/2"], ["-G", "0,1"], ["-Z"]])
def test_combinations_that_are_not_built(tmp_path, args):
    for opt in ("-8", "--siteprefs"):
        p = _run(opt, str(tmp_path / "s.csv"), *args)
        assert p.returncode == 3 and "not built" in p.stderr, p.stderr
        assert not os.path.exists(tmp_path / "s.csv")
