"""GPU parity of the OPTIONAL phases of CSfxArray::AlignReads (chimeric trimming `-c`, microInDels `-a`,
splice junctions `-A`) and of the post-alignment stages they bring with them, through the C ABI of libk4sfx.so:
(1) the vectors the real reference returned (tests/golden/align_ext_*.npz, g3 index), (2) the CPU oracle on fresh inputs,
raw AlignReads and CKAligner::AlignRead level, (3) AutoTrimFlanks / orphan-junction removal against the oracle."""
import glob
import os

import numpy as np
import pytest

import kit4b_amd as k4
import synth
from oracle_bindings import EXT_INDEL, EXT_SPLICE
from test_oracle_ext import CASES, check_ext, ext_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g3(g3_path):
    ix = k4.SfxIndex.open(g3_path)
    ix.set_max_iter(5000)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def g3_el5(g3_el5_path):
    ix = k4.SfxIndex.open(g3_el5_path)
    ix.set_max_iter(5000)
    yield ix
    ix.close()


@pytest.mark.parametrize("case", CASES)
def test_reference_golden_ext(g3, g3_el5, golden_dir, case):
    g = np.load(os.path.join(golden_dir, "align_ext_%s.npz" % case))
    ix = g3_el5 if case.endswith("_el5") else g3
    check_ext(ix.align_reads_ext_batch((g["reads"], g["offs"], g["lens"]), **ext_params(g)), g)


def test_ext_entry_points_refuse_what_they_cannot_report(g3):
    rd = [np.zeros(60, np.uint8)]
    with pytest.raises(k4.K4Error):  # two-segment phases need the k4_seg2 output of the *_ext entry points
        g3.kalign_batch(rd, max_subs=2, max_num_slides=0, min_core_len=8)  # fine ...
        p = k4.AlignParams(2, 20, 20, 5, 8, 1, 0, 1, 0, 10, 0)
        n = 1
        import ctypes as C
        z = np.zeros(16, np.int32)
        h = np.zeros(1, dtype=k4.HIT_DTYPE)
        cat, offs, lens = k4._flatten(rd)
        g3._ck(k4.lib().k4_align_reads_batch(g3.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                             z.ctypes.data, z.ctypes.data + 4, z.ctypes.data + 8, z.ctypes.data + 12, h.ctypes.data))
    with pytest.raises(k4.K4Error):
        g3.align_reads_ext_batch(rd, 2, 20, 20, 5, 8, max_splice_junct_len=10)  # below cMinJunctAlignSep


def _fresh(oracle, tmp_path, seed):
    names, chroms = synth.make_genome([70000, 50000, 30000], seed=seed, repeats=30, repeat_len=300, repeat_div=0.02, n_runs=4,
                                      tandem=4)
    sites = synth.plant_splice_sites(chroms, 50, seed=seed + 1)
    h = oracle.build(names, chroms)
    oracle.set_max_iter(h, 5000)
    path = str(tmp_path / ("x%d.sfx" % seed))
    oracle.write(h, path)
    ix = k4.SfxIndex.open(path)
    ix.set_max_iter(5000)
    return names, chroms, sites, h, ix


def _reads(chroms, sites, rl, seed, n=250):
    reads = synth.make_reads(chroms, n, rl, seed=seed, n_prob=0.03, edge_frac=0.05)[0]
    for k, kind in enumerate(("chimeric", "indel", "splice")):
        reads += synth.make_ext_reads(chroms, n, rl, kind, seed=seed + 10 + k, sites=sites, max_subs=3)
    return reads


def test_fresh_inputs_vs_oracle_raw(oracle, tmp_path):
    names, chroms, sites, h, ix = _fresh(oracle, tmp_path, 1234)
    for rl, kw in ((100, dict(tot_mm=2, core_len=33, core_delta=33, max_slides=8, min_core_len=8)),
                   (151, dict(tot_mm=5, core_len=25, core_delta=25, max_slides=12, min_core_len=9, mm_delta=2)),
                   (64, dict(tot_mm=3, core_len=16, core_delta=16, max_slides=6, min_core_len=8)),
                   (300, dict(tot_mm=6, core_len=42, core_delta=42, max_slides=24, min_core_len=8))):
        reads = _reads(chroms, sites, rl, 7 * rl)
        for mh, ext in ((1, dict(min_chimeric_len=50)), (5, dict(min_chimeric_len=30, micro_indel_len=20)),
                        (1, dict(micro_indel_len=7, max_splice_junct_len=3500)), (2, dict(min_chimeric_len=65, max_splice_junct_len=600)),
                        (1, dict(strand=2, min_chimeric_len=45, micro_indel_len=12, max_splice_junct_len=2000))):
            a = ix.align_reads_ext_batch(reads, max_hits=mh, **kw, **ext)
            b = oracle.align_reads_ext_batch(h, reads, max_hits=mh, **kw, **ext)
            check_ext(a, b)
    ix.close()
    oracle.close(h)


def test_fresh_inputs_vs_oracle_kalign_level_and_post_stages(oracle, tmp_path):
    names, chroms, sites, h, ix = _fresh(oracle, tmp_path, 4321)
    rng = np.random.default_rng(3)
    reads = []
    for rl in (100, 75, 126):
        reads += _reads(chroms, sites, rl, 11 * rl, n=200)
    # several reads over the same junctions so that some survive the orphan filters
    reads += synth.make_ext_reads(chroms, 600, 100, "splice", seed=77, sites=sites[:12], max_subs=1)
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    for kw in (dict(max_subs=2, min_chimeric_len=50), dict(max_subs=3, micro_indel_len=15, max_splice_junct_len=4000),
               dict(max_subs=5, min_edit_dist=2, min_chimeric_len=40, micro_indel_len=20, max_splice_junct_len=3000, max_ml=3, pe_mode=1)):
        a = ix.kalign_ext_batch(reads, **kw)
        b = oracle.kalign_ext_batch(h, reads, **kw)
        for k in ("out", "hits", "seg2"):
            d = a[k] != b[k]
            if d.ndim > 1:
                d = d.any(axis=1)
            assert not d.any(), (k, np.nonzero(d)[0][:5], a[k][d][:2], b[k][d][:2])
        if kw.get("max_ml", 1) != 1:
            continue
        mfe = 3
        o_out, o_hits = b["out"].copy(), b["hits"].copy()
        ne = oracle.auto_trim_flanks(h, reads, o_out, o_hits, b["seg2"], mfe)
        ns = oracle.remove_orphan_juncts(EXT_SPLICE, o_out, o_hits, b["seg2"])
        ni = oracle.remove_orphan_juncts(EXT_INDEL, o_out, o_hits, b["seg2"])
        g_out, g_hits, cnt = ix.post_stages(reads, a["out"], a["hits"], a["seg2"], min_flank_exacts=mfe, orphan_splice=True,
                                            orphan_indel=True)
        assert cnt == {"trim": ne, "splice": ns, "indel": ni}
        assert np.array_equal(g_out, o_out) and np.array_equal(g_hits, o_hits)
    ix.close()
    oracle.close(h)


# ---- the orphan-junction stage at small selected counts ---------------------------------------------------------------------------
def _junction_results(m, flag, seed):
    """(out, hits, seg2) of SE results with exactly m accepted reads that carry `flag`, on two sequences: single junctions, groups
    of two or three reads whose seg-0 ends and seg-1 starts chain within 3 bp, pairs that agree at one end only; between them
    accepted reads without a junction, accepted reads with the other junction kind, and reads that carry `flag` but were not
    accepted.  The last junction of sequence 1 and the first of sequence 2 lie 1 bp apart in both coordinates."""
    rng = np.random.default_rng(seed)
    other = EXT_INDEL if flag == EXT_SPLICE else EXT_SPLICE
    sites = {0: [], 1: [1], 2: [2], 3: [1, 2]}.get(m)  # reads per site; -2: a pair that is close at the seg-0 end only
    if sites is None:
        sites, left = [], m
        while left:
            k = int(rng.choice([1, 1, 2, 3, -2]))
            sites.append(k if abs(k) <= left else 1)
            left -= abs(sites[-1])
    half = len(sites) // 2  # sites of sequence 1; the two next to the boundary get one read each, the others go to the end
    if m > 3:
        for q in (half - 1, half):
            sites += [1] * (abs(sites[q]) - 1)
            sites[q] = 1
    assert sum(abs(k) for k in sites) == m
    junct = []  # (chrom, seg-0 end, seg-1 start)
    for q, k in enumerate(sites):
        chrom = 1 if q < half or len(sites) < 2 else 2
        e0, s1 = 5000 + 1000 * q, 9000 + 1000 * q
        if q == half and m > 3:
            e0, s1 = 5000 + 1000 * (q - 1) + 1, 9000 + 1000 * (q - 1) + 1
        for _ in range(abs(k)):
            junct.append((chrom, e0, s1))
            e0 += int(rng.integers(-3, 4))
            s1 += int(rng.integers(-3, 4)) if k > 0 else 4 + int(rng.integers(0, 50))
    n_plain, n_other, n_rejected = m // 2 + 5, m // 4 + 3, m // 4 + 3
    n = m + n_plain + n_other + n_rejected
    out = np.zeros(n, k4.RESULT_DTYPE)
    hits = np.zeros((n, 1), k4.HIT_DTYPE)
    seg2 = np.zeros(n, k4.SEG2_DTYPE)
    out["hit_rslt"], out["inst"], out["nar"], out["num_hits"] = 1, 1, 1, 1
    hits["chrom_id"][:, 0] = rng.integers(1, 3, n)
    hits["match_loci"][:, 0] = rng.integers(5000, 300000, n)
    hits["match_len"][:, 0] = 40
    hits["strand"][:, 0] = np.where(rng.random(n) < 0.5, ord("+"), ord("-"))
    for k, (chrom, e0, s1) in enumerate(junct):
        hits["chrom_id"][k, 0], hits["match_loci"][k, 0] = chrom, e0 - 39
        seg2["chrom_id"][k], seg2["match_loci"][k], seg2["match_len"][k], seg2["read_ofs"][k] = chrom, s1, 60, 40
    hits["reserved"][:m, 0] = flag
    a = m + n_plain
    hits["reserved"][a:a + n_other, 0] = other
    seg2["match_loci"][a:], seg2["match_len"][a:] = hits["match_loci"][a:, 0] + 500, 60
    hits["reserved"][a + n_other:, 0] = flag  # junction reads at the loci of accepted ones that something earlier turned down
    out["nar"][a + n_other:] = rng.choice([0, 3, 6], n_rejected)
    out["num_hits"][a + n_other:] = 0
    for k in range(min(m, n_rejected)):
        hits["chrom_id"][a + n_other + k, 0], hits["match_loci"][a + n_other + k, 0] = hits["chrom_id"][k, 0], hits["match_loci"][k, 0]
        seg2["match_loci"][a + n_other + k] = seg2["match_loci"][k]
    order = rng.permutation(n)
    return out[order], hits[order], seg2[order]


@pytest.mark.parametrize("m,flag", [(m, EXT_SPLICE) for m in (0, 1, 2, 3, 255, 256, 257)] + [(1, EXT_INDEL), (257, EXT_INDEL)])
def test_orphan_juncts_small_counts_vs_oracle(oracle, g3, m, flag):
    """k4_remove_orphan_juncts_dev where its control flow branches: nothing selected, a lone junction (no sort, no neighbour
    test), two and three, and one block of 256 threads more or less."""
    out, hits, seg2 = _junction_results(m, flag, 1000 + m)
    assert int(((out["nar"] == 1) & ((hits["reserved"][:, 0] & flag) != 0)).sum()) == m
    o_out, o_hits = out.copy(), hits.copy()
    want = oracle.remove_orphan_juncts(flag, o_out, o_hits, seg2)
    if m > 3:  # the input has both outcomes
        assert m // 4 < want < m - m // 4
    reads = [np.zeros(4, np.uint8)] * len(out)
    splice = flag == EXT_SPLICE
    g_out, g_hits, cnt = g3.post_stages(reads, out, hits, seg2, min_flank_exacts=0, orphan_splice=splice, orphan_indel=not splice)
    print("m %d selected, %d removed (oracle %d)" % (m, list(cnt.values())[0], want))
    assert cnt == {"splice" if splice else "indel": want}
    assert np.array_equal(g_out, o_out) and np.array_equal(g_hits, o_hits)
