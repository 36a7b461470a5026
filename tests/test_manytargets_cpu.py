"""The CPU oracle on an index of 300 targets (tests/manytargets.py), pinned before the GPU tests use it as their yardstick
(test_gpu_manytargets.py): against the vectors the real reference returned (tests/golden/align_mt300_*.npz), against the live
reference where oracle/_ref was built, and the properties that make those inputs worth running -- targets on both sides of
K4_LDS_ENTRIES (128), reads hugging target ends, reads one base too long for a target, byte-identical targets."""
import ctypes as C
import os

import numpy as np
import pytest

import manytargets as mt
from manytargets import NPZ_CASES, RAW_ARGS
from oracle_bindings import Ref, _RefHit, HIT_DTYPE, oracle_kalign_pe, ref_available
from test_oracle_golden import check_against

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def mt300(oracle, tmp_path_factory):
    """(targets, oracle handle, path of the .sfx the oracle wrote) of the 300-target genome"""
    names, chroms = mt.genome(300)
    h = oracle.build(names, chroms, dataset="mt300", threads=4)
    oracle.set_max_iter(h, 5000)
    path = str(tmp_path_factory.mktemp("mt300") / "mt300.sfx")
    oracle.write(h, path)
    yield chroms, h, path
    oracle.close(h)


def test_genome_layout():
    names, chroms = mt.genome(300)
    lens = [len(c) for c in chroms]
    assert 140_000 < sum(lens) < 180_000
    for n in (128, 129):  # a shorter genome is a prefix of the longer one
        _, part = mt.genome(n)
        assert all(np.array_equal(a, b) for a, b in zip(part, chroms)) and len(part) == n
    assert sorted(lens[i] for i in (3, 4, 5)) == sorted(lens[i] for i in (131, 132, 133)) == [1, 7, 40]
    for i, (L, ln) in mt.EXACT.items():
        assert lens[i] == ln and ln in (L, L - 1)
    assert any(i < 128 for i in mt.EXACT) and any(i >= 128 for i in mt.EXACT)
    for a, b in mt.DUPLICATES:
        assert np.array_equal(chroms[a], chroms[b])
    assert mt.DUPLICATES[0][0] < 128 <= mt.DUPLICATES[0][1]
    for i in mt.LONG:
        assert lens[i] == 2500
    for i in mt.N_TAIL:
        assert chroms[i][-1] == 4 and chroms[i][-mt.N_TAIL_LEN - 1] < 4
    assert all(lens[i] >= max(mt.RAW_LENS) for i in mt.end_targets(300))
    assert mt.end_targets(300) == [0, 1, 126, 127, 128, 129, 298, 299] and mt.end_targets(129) == [0, 1, 126, 127, 128]


@pytest.mark.parametrize("case", NPZ_CASES)
def test_oracle_matches_reference_golden_300_targets(oracle, mt300, case):
    chroms, h, _ = mt300
    g = np.load(os.path.join(GOLDEN, "align_%s.npz" % case))
    tm, cl, cd, sl, mcl, md, strand, mh, maxiter = [int(x) for x in g["params"]]
    oracle.set_max_iter(h, maxiter)
    res = oracle.align_reads_batch(h, (g["reads"], g["offs"], g["lens"]), tm, cl, cd, sl, mcl, md, strand, mh)
    check_against(res, g, mh)
    acc = g["rslt"] == 1
    assert 4 * (g["hits"][acc, 0]["chrom_id"] > 128).sum() >= acc.sum() > 1000
    if mh > 1:  # reads on the byte-identical targets: both ids, in the stored order
        two = acc & (g["inst"] == 2)
        ids = {tuple(sorted((int(a), int(b)))) for a, b in zip(g["hits"][two, 0]["chrom_id"], g["hits"][two, 1]["chrom_id"])}
        assert {(a + 1, b + 1) for a, b in mt.DUPLICATES} <= ids


@pytest.mark.parametrize("read_len", mt.RAW_LENS)
@pytest.mark.parametrize("max_hits", [1, 10])
def test_crafted_reads_at_target_ends(oracle, mt300, read_len, max_hits):
    """what the inputs of the GPU tests must show, on the oracle's own results"""
    chroms, h, _ = mt300
    reads, groups = mt.raw_batch(chroms, 2000, read_len, seed=read_len + max_hits)
    r = oracle.align_reads_batch(h, reads, *RAW_ARGS[read_len], 0, 1, 0, max_hits)
    hit0 = r["hits"][:, 0]
    acc = r["rslt"] == 1
    assert 4 * (acc & (hit0["chrom_id"] > 128)).sum() >= acc.sum() > 1000
    for name in ("ends", "exact"):  # accepted at the truth locus, target ends and whole targets on both sides of 128
        a, b, truth = groups[name]
        assert b - a == (32 if name == "ends" else 4)
        assert (truth[:, 0] > 128).any() and (truth[:, 0] <= 128).any()
        assert (r["rslt"][a:b] == 1).all() and (r["inst"][a:b] == 1).all(), name
        assert np.array_equal(hit0["chrom_id"][a:b], truth[:, 0]) and np.array_equal(hit0["match_loci"][a:b], truth[:, 1])
        assert np.array_equal(hit0["strand"][a:b] == ord("-"), truth[:, 2] == 1) and (hit0["mismatches"][a:b] == 0).all()
    a, b, rows = groups["beyond"]  # one base past an end, and the targets of read length - 1: never placed there
    assert b - a == 40 and (rows[:, 0] > 128).any() and (rows[:, 0] <= 128).any()
    short = np.isin(rows[:, 0] - 1, [i for i, (L, ln) in mt.EXACT.items() if ln == L - 1])
    assert short.sum() == 8
    for k in range(a, b):
        nh = min(int(r["inst"][k]), max_hits) if r["rslt"][k] in (1, 2, 3) else 0
        assert not (r["hits"][k, :nh]["chrom_id"] == rows[k - a, 0]).any(), (k, r["hits"][k, :nh])
    a, b, pair = groups["dup"]
    assert (r["inst"][a:b] == 2).all() and b - a == 200
    if max_hits > 1:
        assert (r["rslt"][a:b] == 1).all()
        ids = np.sort(np.stack([r["hits"][a:b, 0]["chrom_id"], r["hits"][a:b, 1]["chrom_id"]], 1), 1)
        assert np.array_equal(ids, np.array([[mt.DUPLICATES[k][0] + 1, mt.DUPLICATES[k][1] + 1] for k in pair]))
        for f in ("match_loci", "strand", "mismatches", "match_len"):
            assert np.array_equal(r["hits"][a:b, 0][f], r["hits"][a:b, 1][f]), f
    else:
        assert (r["rslt"][a:b] == 3).all()  # more instances than slots


def test_mixed_and_paired_inputs_reach_the_targets_above_128(oracle, mt300):
    chroms, h, _ = mt300
    reads = mt.mixed_batch(chroms, 11)
    general = np.array([(rd > 3).any() or len(rd) > 512 for rd in reads])  # the reads the general kernel answers
    for kw in (dict(max_subs=0), dict(max_subs=2), dict(max_subs=5), dict(max_subs=5, max_ml=10, pe_mode=1), dict(max_subs=3, max_ml=10, pe_mode=4)):
        r = oracle.kalign_batch(h, reads, **kw)
        acc = r["out"]["nar"] == 1
        high = acc & (r["hits"][:, 0]["chrom_id"] > 128)
        assert 4 * high.sum() >= acc.sum() and (high & general).sum() > (0 if kw["max_subs"] == 0 else 100), kw
    pe1, pe2, kind, _ = mt.pe_batch(chroms, 2500)
    for pe_mode in (1, 2, 3, 4):
        o = oracle_kalign_pe(oracle, h, pe1, pe2, pe_mode=pe_mode, pair_min_len=150, pair_max_len=500, max_subs=2)
        o1, o2 = o[0::2], o[1::2]
        if pe_mode in (1, 3):  # mates placed by the rescue on targets with id > 128, most of them the pairs made for it
            res = (o["rescued"] > 0) & (o["nar"] == 1) & (o["hit"]["chrom_id"] > 128)
            assert res.sum() > 200 and ((o1["rescued"] + o2["rescued"])[kind == 1] > 0).sum() > 150
        else:
            assert o["rescued"].sum() == 0
        both = (o1["nar"] == 1) & (o2["nar"] == 1)
        cross = both & (o1["hit"]["chrom_id"] != o2["hit"]["chrom_id"])
        assert cross.sum() == ((both & (kind == 2)).sum() if pe_mode in (3, 4) else 0)
        assert cross.sum() > (200 if pe_mode in (3, 4) else -1)
        assert (o1["pe_aligned"] & (o1["hit"]["chrom_id"] > 128)).sum() > 500


# ---- the live reference ----------------------------------------------------------------------------------------------
@pytest.mark.skipif(not ref_available(), reason="oracle/_ref not built (no /root/reference here)")
def test_oracle_matches_live_reference_300_targets(oracle, mt300):
    """CSfxArray::AlignReads read for read, every read length class and both hit limits, on the index file the oracle wrote"""
    chroms, h, path = mt300
    R = Ref()
    hr = R.open(path, 5000, 0)
    oracle.set_max_iter(h, 5000)
    for read_len in mt.RAW_LENS:
        for max_hits in (1, 10):
            reads, _ = mt.raw_batch(chroms, 600, read_len, seed=7 * read_len + max_hits)
            ro = oracle.align_reads_batch(h, reads, *RAW_ARGS[read_len], 0, 1, 0, max_hits)
            rr = R.align_reads_batch(hr, reads, *RAW_ARGS[read_len], 0, 1, 0, max_hits)
            check_against(ro, rr, max_hits)
    R.close(hr)


@pytest.mark.skipif(not ref_available(), reason="oracle/_ref not built (no /root/reference here)")
def test_oracle_mate_rescue_matches_live_reference_300_targets(oracle, mt300):
    """CSfxArray::AlignPairedRead (the PE entry point: mate rescue next to an anchor) with anchors on targets on both sides of 128,
    the repeat targets and the target ends among them; insert windows below 1000 loci (the reference has no behaviour above:
    test_oracle_sam_golden.py::test_reference_dies_on_wide_rescue_window)."""
    chroms, h, path = mt300
    R = Ref()
    hr = R.open(path, 5000, 0)
    fr = R.L.k4ref_align_paired_read
    fr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_int] * 9 + [C.c_void_p, C.POINTER(_RefHit)]
    fo = oracle.L.k4o_align_paired_read
    fo.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(300)
    L = 100
    targets = [t for t in list(mt.REPEAT_TARGETS) + mt.end_targets(300) + list(rng.integers(0, 300, 60)) if len(chroms[t]) >= 450]
    n_placed = n_high = 0
    for t, b3, anti, a_start, a_end, lo, hi, max_mm, mate in mt.rescue_calls(chroms, targets, rng, read_len=L):
        buf_r, buf_o = mate.copy(), mate.copy()
        xr, xo = _RefHit(), np.zeros(1, dtype=HIT_DTYPE)
        r_ref = fr(hr, b3, anti, t + 1, a_start, a_end, lo, hi, max_mm, 1, L, 0, L // (max_mm + 1), L // (max_mm + 1), 8,
                   buf_r.ctypes.data, C.byref(xr))
        r_o = fo(h, b3, anti, t + 1, a_start, a_end, lo, hi, max_mm, L, buf_o.ctypes.data, xo.ctypes.data)
        assert r_ref == r_o, (t, a_start, b3, anti, r_ref, r_o)
        if r_ref == 1:
            got = (int(xo[0]["chrom_id"]), int(xo[0]["match_loci"]), int(xo[0]["match_len"]), int(xo[0]["strand"]), int(xo[0]["mismatches"]))
            assert got == (xr.chrom_id, xr.match_loci, xr.match_len, xr.strand, xr.mismatches), (t, a_start, b3, anti)
            n_placed += 1
            n_high += t >= 128
    assert n_placed > 150 and n_high > 60
    R.close(hr)
