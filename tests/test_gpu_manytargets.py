"""Alignment, pairing and record formatting on indexes with more than K4_LDS_ENTRIES (128) targets (-m gpu).

Up to 128 targets the step kernels and the general kernel search a copy of the entry table in LDS; above, both fall through to
k4d_map_entry over global memory and the general kernel lays out its LDS without the table; the pairing / rescue kernel always
calls k4d_map_entry.  Every case here runs on 128 (the LDS table full to its last slot), 129 (the first size on the global
path), 300 or 12 000 targets and compares with the CPU oracle, which test_manytargets_cpu.py pins to the reference on the same
300 targets, or with the reference's own vectors (tests/golden/align_mt300_*.npz)."""
import ctypes as C
import json
import lzma
import os
import struct
import subprocess

import numpy as np
import pytest

import manytargets as mt
from manytargets import NPZ_CASES, RAW_ARGS
from oracle_bindings import oracle_kalign_pe
from test_gpu_parity import check_against
from test_gpu_workspace import RESCUE_TASK_DTYPE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MT300 = json.load(open(os.path.join(GOLDEN, "mt300_cases.json")))
# (targets, layout): 4- / 5-byte suffix elements, 16- / 12-byte k-mer table entries; the layouts on the 129 and 300 sizes only
CONFIGS = [(128, "el4"), (12000, "el4")] + [(n, lay) for n in (129, 300) for lay in ("el4", "el5", "el4_kt32", "el5_kt32")]
IDS = ["%d-%s" % c for c in CONFIGS]


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


class _Genomes:
    """the genomes, their oracle indexes (one per size and element size) and the oracle's results, each made once"""

    def __init__(self, oracle):
        self.oracle, self.g, self.h, self.memo = oracle, {}, {}, {}

    def chroms(self, n):
        if n not in self.g:
            self.g[n] = mt.genome(n) if n <= 300 else mt.small_genome(n)
        return self.g[n]

    def handle(self, n, el=4):
        if (n, el) not in self.h:
            names, chroms = self.chroms(n)
            self.h[(n, el)] = self.oracle.build(names, chroms, dataset="mt%d" % n, force_el=el if el == 5 else 0, threads=8)
            self.oracle.set_max_iter(self.h[(n, el)], 5000)
        return self.h[(n, el)]

    def want(self, key, fn):
        """the oracle's answer to `key` (the same whatever the layout of the device index)"""
        if key not in self.memo:
            self.memo[key] = fn(self.handle(key[0]))
        return self.memo[key]

    def close(self):
        for h in self.h.values():
            self.oracle.close(h)


@pytest.fixture(scope="module")
def genomes(oracle):
    g = _Genomes(oracle)
    yield g
    g.close()


def _open(k4, genomes, monkeypatch, n, layout):
    """the device index of the n-target genome: 12 000 targets sorted on the device (as test_gpu_stats.py does), the others from
    the oracle's suffix array"""
    import torch

    el = 5 if layout.startswith("el5") else 4
    if layout.endswith("kt32"):  # the {lb, pos0, sig} form a device short of memory falls back to (k4_index.hip: open_common)
        monkeypatch.setenv("K4_FORCE_KTAB64", "0")
    names, chroms = genomes.chroms(n)
    ents = k4.make_entries(names, [len(c) for c in chroms])
    oracle, h = genomes.oracle, genomes.handle(n, el)
    cat = oracle.concat_len(h)
    if n > 300:
        d_seq = torch.from_numpy(np.array(oracle.seq(h))).cuda()
        sa = torch.empty(cat, dtype=torch.int32, device="cuda")
        k4.build_sa_device(cat, 4, d_seq.data_ptr(), sa.data_ptr())
        ix = k4.SfxIndex.from_device(cat, 4, d_seq.data_ptr(), sa.data_ptr(), ents, keep=(sa, d_seq))
    else:
        sa_raw = np.ctypeslib.as_array(C.cast(oracle.L.k4o_sa_bytes(h), C.POINTER(C.c_uint8)), shape=(cat * el,))
        ix = k4.SfxIndex.from_host(np.array(oracle.seq(h)), sa_raw, el, ents, dataset="mt%d" % n)
    info = ix.info()
    assert info["n_entries"] == n and info["sfx_el_size"] == el
    ix.set_max_iter(5000)
    return ix, chroms


def _high(hit0, accepted):
    """accepted reads whose reported hit lies on a target with id > 128"""
    return int((accepted & (hit0["chrom_id"] > 128)).sum())


def _general(reads):
    """the reads the general kernel answers: an N in them, or over 512 bp"""
    return np.array([(rd > 3).any() or len(rd) > 512 for rd in reads])


@pytest.mark.parametrize("n,layout", CONFIGS, ids=IDS)
def test_align_reads_batch_vs_oracle(k4, genomes, monkeypatch, n, layout):
    """Raw AlignReads, uniform-length batches of 100 / 150 / 250 / 400 bp (the step kernels' NCH 4, 5, 8 and 16) with one and ten hit
    slots; reads at locus 0 and at the last base of the targets around 128 and of the first and last targets, whole targets, reads
    one base too long for a target, reads on byte-identical targets; stale hit slots included."""
    ix, chroms = _open(k4, genomes, monkeypatch, n, layout)
    try:
        for read_len in mt.RAW_LENS:
            for max_hits in (1, 10):
                reads, groups = mt.raw_batch(chroms, 2000, read_len, seed=read_len + max_hits, crafted=n <= 300)
                args = RAW_ARGS[read_len] + (0, 1, 0, max_hits)
                want = genomes.want((n, "raw", read_len, max_hits), lambda h: genomes.oracle.align_reads_batch(h, reads, *args, threads=8))
                got = ix.align_reads_batch(reads, *args)
                check_against(got, want, max_hits, "%d targets, %d bp, %d slots" % (n, read_len, max_hits))
                acc = want["rslt"] == 1
                high = _high(want["hits"][:, 0], acc)
                print("raw n=%d %s len=%d max_hits=%d: %d reads, %d accepted, %d on id > 128" % (n, layout, read_len, max_hits, len(reads), acc.sum(), high))
                assert acc.sum() > 1000 and (high > 0 if n > 128 else high == 0)
                a, b, truth = groups["ends"]
                assert (b > a or n > 300) and (want["rslt"][a:b] == 1).all() and np.array_equal(got["hits"][a:b, 0]["match_loci"], truth[:, 1])
        assert ix.counters()["n_slow"] > 0  # (the reads with N)
    finally:
        ix.close()


KALIGN_KW = [dict(max_subs=0), dict(max_subs=2), dict(max_subs=5), dict(max_subs=5, max_ml=10, pe_mode=1), dict(max_subs=3, max_ml=10, pe_mode=4)]


@pytest.mark.parametrize("n,layout", CONFIGS, ids=IDS)
def test_kalign_batch_vs_oracle(k4, genomes, monkeypatch, n, layout):
    """AlignRead over 36 to 2 000 bp reads in one batch, many with N: the general kernel (its LDS layout without the entry table above
    128 targets) and the reads over 512 bp next to every step-kernel class; `-s0`, `-s2`, `-s5`, multi-aligned reads kept (pe_mode 1)
    and LocateBestMatches (pe_mode 4)."""
    ix, chroms = _open(k4, genomes, monkeypatch, n, layout)
    try:
        reads = mt.mixed_batch(chroms, 11, crafted=n <= 300)
        general = _general(reads)
        for kw in KALIGN_KW:
            want = genomes.want((n, "kalign", tuple(sorted(kw.items()))), lambda h: genomes.oracle.kalign_batch(h, reads, threads=8, **kw))
            ix.reset_counters()
            got = ix.kalign_batch(reads, **kw)
            assert ix.counters()["n_slow"] > 0
            for f in ("hit_rslt", "inst", "low_mm", "nxt_mm", "nar", "num_hits"):
                bad = np.nonzero(want["out"][f] != got["out"][f])[0]
                assert len(bad) == 0, (kw, f, bad[:5], want["out"][f][bad[:5]], got["out"][f][bad[:5]])
            mh = max(1, kw.get("max_ml", 1))
            for i in range(len(reads)):
                r = want["out"][i]
                nh = min(int(r["inst"]), mh) if r["hit_rslt"] in (1, 2, 3) else 0
                assert np.array_equal(want["hits"][i, :nh], got["hits"][i, :nh]), (kw, i)
            acc = want["out"]["nar"] == 1
            hit0 = want["hits"][:, 0]
            print("kalign n=%d %s %s: %d reads, %d accepted, %d on id > 128, %d of those answered by the general kernel" % (
                n, layout, kw, len(reads), acc.sum(), _high(hit0, acc), _high(hit0, acc & general)))
            # (`-s0`: an N is a mismatch, so the general kernel's accepted reads are the exact ones over 512 bp: none fits a target of the
            # 12 000, and the one target above 128 of the 129 draws too few to count on)
            if n == 300 or (n > 128 and kw["max_subs"]):
                assert _high(hit0, acc & general) > 0
    finally:
        ix.close()


@pytest.mark.parametrize("n,layout", [(129, "el4"), (300, "el4"), (300, "el5_kt32"), (12000, "el4")], ids=lambda v: str(v))
def test_best_matches_raw_call_vs_oracle(k4, genomes, monkeypatch, n, layout):
    """k4_best_matches_batch (LocateBestMatches, `-N`): return value, instance count and the sorted hit list"""
    ix, chroms = _open(k4, genomes, monkeypatch, n, layout)
    oracle, h = genomes.oracle, genomes.handle(n)
    L = oracle.L
    L.k4o_locate_best_matches.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_int,
                                                                         C.c_void_p]
    try:
        reads = mt.raw_batch(chroms, 1500, 100, seed=81, crafted=n <= 300)[0]
        for max_hits, tot_mm in ((6, 3), (1, 0)):
            g = ix.best_matches_batch(reads, tot_mm, 25, 25, 8, max_hits=max_hits)
            n_high = 0
            for i, rd in enumerate(reads):
                buf = np.ascontiguousarray(rd, dtype=np.uint8).copy()
                hits = np.zeros(max_hits + 1, dtype=g["hits"].dtype)
                inst = C.c_int(0)
                r = L.k4o_locate_best_matches(h, tot_mm, 25, 25, 8, 0, buf.ctypes.data, len(buf), max_hits, C.byref(inst), hits.ctypes.data, 5000, None)
                assert (r, inst.value) == (int(g["rslt"][i]), int(g["inst"][i])), (i, r, inst.value, g["rslt"][i], g["inst"][i])
                assert np.array_equal(hits[: inst.value], g["hits"][i][: inst.value]), i
                assert not g["hits"][i][inst.value:].view(np.uint8).any()
                n_high += inst.value > 0 and hits[0]["chrom_id"] > 128
            print("best matches n=%d %s max_hits=%d: %d reads, %d with their first hit on id > 128" % (n, layout, max_hits, len(reads), n_high))
            assert n_high > (100 if n >= 300 else 0)  # (129 targets: one target above 128, a 129th of the reads)
    finally:
        ix.close()


@pytest.mark.parametrize("layout", ["el4", "el5", "el4_kt32", "el5_kt32"])
@pytest.mark.parametrize("case", NPZ_CASES)
def test_golden_vectors_from_reference_300_targets(k4, genomes, monkeypatch, case, layout):
    """what the reference's own AlignReads returned on the 300-target index (tests/golden/make_golden_manytargets.py)"""
    ix, _ = _open(k4, genomes, monkeypatch, 300, layout)
    try:
        g = np.load(os.path.join(GOLDEN, "align_%s.npz" % case))
        tm, cl, cd, sl, mcl, md, strand, mh, maxiter = [int(x) for x in g["params"]]
        ix.set_max_iter(maxiter)
        res = ix.align_reads_batch((g["reads"], g["offs"], g["lens"]), tm, cl, cd, sl, mcl, md, strand, mh)
        check_against(res, g, mh, case)
        acc = g["rslt"] == 1
        print("golden %s %s: %d reads, %d accepted, %d on id > 128" % (case, layout, len(g["lens"]), acc.sum(), _high(g["hits"][:, 0], acc)))
    finally:
        ix.close()


@pytest.mark.parametrize("pe_mode", [1, 2, 3, 4])
@pytest.mark.parametrize("n,layout", [(128, "el4"), (129, "el4"), (300, "el4"), (300, "el5_kt32"), (12000, "el4")], ids=lambda v: str(v))
def test_pe_flow_vs_oracle(k4, genomes, monkeypatch, n, layout, pe_mode):
    """`-U1` to `-U4`: the pairing kernel and the mate rescue (both call k4d_map_entry whatever the target count) on ordinary pairs, on
    pairs whose one end can only be placed by the rescue on a target with id > 128, and on pairs whose ends lie on different
    targets."""
    ix, chroms = _open(k4, genomes, monkeypatch, n, layout)
    try:
        if n <= 300:
            pe1, pe2, kind, _ = mt.pe_batch(chroms, 2500)
            kw = dict(pe_mode=pe_mode, pair_min_len=150, pair_max_len=500, max_subs=2)
        else:
            pe1, pe2, kind, _ = mt.pe_batch(chroms, 2500, read_len=75, frag_min=160, frag_max=300, crafted=False)
            kw = dict(pe_mode=pe_mode, pair_min_len=120, pair_max_len=350, max_subs=3)
        o = genomes.want((n, "pe", pe_mode), lambda h: oracle_kalign_pe(genomes.oracle, h, pe1, pe2, threads=8, **kw))
        g = ix.kalign_pe_batch(pe1, pe2, **kw)
        for f in ("nar", "num_hits", "inst", "low_mm", "pe_aligned", "rescued"):
            bad = np.nonzero(g[f] != o[f])[0]
            assert len(bad) == 0, (f, bad[:6], g[f][bad[:6]], o[f][bad[:6]])
        acc = g["nar"] == 1
        assert np.array_equal(g["hit"][acc], o["hit"][acc])
        high = acc & (o["hit"]["chrom_id"] > 128)
        resc = high & (o["rescued"] > 0)
        o1, o2 = o[0::2], o[1::2]
        cross = (o1["nar"] == 1) & (o2["nar"] == 1) & (o1["hit"]["chrom_id"] != o2["hit"]["chrom_id"])
        print("pe n=%d %s -U%d: %d pairs, %d ends accepted, %d on id > 128, %d of those rescued, %d pairs across targets" % (
            n, layout, pe_mode, len(pe1), acc.sum(), high.sum(), resc.sum(), cross.sum()))
        assert acc.sum() > 1000 and (high.sum() > 500 if n > 129 else high.sum() > 0 if n == 129 else high.sum() == 0)
        if n == 300:
            assert resc.sum() > (200 if pe_mode in (1, 3) else -1) and cross.sum() > (200 if pe_mode in (3, 4) else -1)
    finally:
        ix.close()


@pytest.mark.parametrize("n,layout", [(129, "el4"), (300, "el4"), (300, "el5_kt32"), (12000, "el4")], ids=lambda v: str(v))
def test_mate_rescue_batch_vs_oracle(k4, genomes, monkeypatch, n, layout):
    """k4_mate_rescue_batch (the k4k_mate_rescue kernel on its own: AlignPairedRead next to a given anchor) against the oracle's
    AlignPairedRead, call for call: anchors on targets on both sides of 128, the repeat targets and the first and last targets
    among them, fragments flush with the target ends, mates within and beyond the allowed substitutions.  On 300 targets these
    are the calls on which test_manytargets_cpu.py compares the oracle with the reference."""
    ix, chroms = _open(k4, genomes, monkeypatch, n, layout)
    fo = genomes.oracle.L.k4o_align_paired_read
    fo.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]
    try:
        rng = np.random.default_rng(300)
        if n <= 300:
            L = 100
            targets = [t for t in list(mt.REPEAT_TARGETS) + mt.end_targets(n) + list(rng.integers(0, n, 60)) if t < n and len(chroms[t]) >= 450]
            calls = mt.rescue_calls(chroms, targets, rng, read_len=L)
        else:
            L = 75
            calls = mt.rescue_calls(chroms, [0, 127, 128, n - 1] + list(rng.integers(0, n, 200)), rng, per_target=5, read_len=L, lo=100, hi=350)
        tasks = np.zeros(len(calls), dtype=RESCUE_TASK_DTYPE)
        for k, (t, b3, anti, a_start, a_end, lo, hi, max_mm, mate) in enumerate(calls):
            tasks[k] = (t + 1, a_start, a_end, L, k * L, b3, anti, lo, hi, max_mm, 0)
        cat = np.ascontiguousarray(np.concatenate([c[-1] for c in calls]), dtype=np.uint8)
        rslt = np.full(len(calls), -99, dtype=np.int32)
        hits = np.zeros(len(calls), dtype=k4.HIT_DTYPE)
        ix._ck(k4.lib().k4_mate_rescue_batch(ix.h, len(calls), tasks.ctypes.data, cat.ctypes.data, len(cat), rslt.ctypes.data, hits.ctypes.data))
        h = genomes.handle(n)
        n_placed = n_high = 0
        for k, (t, b3, anti, a_start, a_end, lo, hi, max_mm, mate) in enumerate(calls):
            buf, xo = mate.copy(), np.zeros(1, dtype=k4.HIT_DTYPE)
            r = fo(h, b3, anti, t + 1, a_start, a_end, lo, hi, max_mm, L, buf.ctypes.data, xo.ctypes.data)
            assert r == rslt[k], (k, calls[k][:8], r, rslt[k])
            if r == 1:
                assert xo[0].tobytes() == hits[k].tobytes(), (k, calls[k][:8], xo[0], hits[k])
                assert xo[0]["chrom_id"] == t + 1
                n_placed += 1
                n_high += t >= 128
            else:
                assert not hits[k:k + 1].view(np.uint8).any(), (k, calls[k][:8])
        print("mate rescue n=%d %s: %d calls, %d mates placed, %d of them on id > 128" % (n, layout, len(calls), n_placed, n_high))
        assert n_placed > 150 and len(calls) - n_placed > 50 and n_high > (60 if n >= 300 else 0)
        if n > 300:
            return
        # chimeric mode (the kernel's other LDS size): windows of 1000 loci and more take their candidates from the suffix array and
        # map each to its target with k4d_map_entry
        calls = mt.chimeric_rescue_calls(chroms, rng)
        mcl, cl, cd = mt.RESCUE_CHIMERIC
        tasks = np.zeros(len(calls), dtype=RESCUE_TASK_DTYPE)
        for k, (t, b3, anti, a_start, a_end, lo, hi, max_mm, mate) in enumerate(calls):
            tasks[k] = (t + 1, a_start, a_end, L, k * L, b3, anti, lo, hi, max_mm, mcl | cl << 8 | cd << 20)
        cat = np.ascontiguousarray(np.concatenate([c[-1] for c in calls]), dtype=np.uint8)
        rslt = np.full(len(calls), -99, dtype=np.int32)
        hits = np.zeros(len(calls), dtype=k4.HIT_DTYPE)
        ix._ck(k4.lib().k4_mate_rescue_batch(ix.h, len(calls), tasks.ctypes.data, cat.ctypes.data, len(cat), rslt.ctypes.data, hits.ctypes.data))
        n_placed = n_high = n_trimmed = 0
        for k, (t, b3, anti, a_start, a_end, lo, hi, max_mm, mate) in enumerate(calls):
            r, xo = genomes.oracle.align_paired_read_x(h, b3, anti, t + 1, a_start, a_end, lo, hi, max_mm, mate, mcl, cl, cd)
            assert r == rslt[k], (k, calls[k][:8], r, rslt[k])
            if r == 1:
                assert xo.tobytes() == hits[k].tobytes(), (k, calls[k][:8], xo, hits[k])
                n_placed += 1
                n_high += t >= 128
                n_trimmed += (int(xo["reserved"]) >> 24) & 1
            else:
                assert not hits[k:k + 1].view(np.uint8).any(), (k, calls[k][:8])
        print("chimeric mate rescue n=%d %s: %d calls, %d mates placed, %d of them on id > 128, %d trimmed" % (n, layout, len(calls), n_placed,
                                                                                                            n_high, n_trimmed))
        assert n_placed > 30 and n_trimmed > 10 and (n_high > 10 if n >= 300 else True)
    finally:
        ix.close()


def test_chimeric_reads_from_targets_above_128(k4, genomes, monkeypatch):
    """`-c50` (k4_kalign_ext_batch): the chimeric phase runs in the general kernel for every read it takes up"""
    ix, chroms = _open(k4, genomes, monkeypatch, 300, "el4")
    try:
        reads = mt.chimeric_reads(chroms, 1500, 100) + mt.raw_batch(chroms, 500, 100, seed=5)[0]
        kw = dict(max_subs=2, min_chimeric_len=50)
        want = genomes.want((300, "chimeric"), lambda h: genomes.oracle.kalign_ext_batch(h, reads, threads=8, **kw))
        got = ix.kalign_ext_batch(reads, **kw)
        for k in ("out", "hits", "seg2"):
            d = want[k] != got[k]
            d = d.any(axis=1) if d.ndim > 1 else d
            assert not d.any(), (k, np.nonzero(d)[0][:5])
        acc = want["out"]["nar"] == 1
        chim = acc & ((want["hits"][:, 0]["reserved"] >> 24) & 1 > 0)
        print("chimeric: %d reads, %d accepted, %d trimmed placements, %d of them on id > 128" % (len(reads), acc.sum(), chim.sum(),
                                                                                                 _high(want["hits"][:, 0], chim)))
        assert _high(want["hits"][:, 0], chim) > 300
    finally:
        ix.close()


@pytest.mark.parametrize("ml_mode", [3, 4])
def test_assign_multi_over_the_duplicate_targets(k4, genomes, monkeypatch, ml_mode):
    """`-r3` / `-r4` (k4_assign_multi_dev) on reads multi-aligned over the byte-identical targets (every locus ties: none may be
    assigned) and over the 12-copy repeat (the copy on target 171 has uniquely aligned neighbours and wins), among unique reads"""
    ix, chroms = _open(k4, genomes, monkeypatch, 300, "el4")
    try:
        reads = mt.raw_batch(chroms, 3000, 100, seed=34)[0] + mt.duplicate_reads(chroms, 300, 100, seed=35)[0] + mt.repeat_reads(chroms, 600, 200)
        kw = dict(max_subs=2, max_ml=16, pe_mode=1)
        want = genomes.want((300, "multi"), lambda h: genomes.oracle.kalign_batch(h, reads, threads=8, **kw))
        got = ix.kalign_batch(reads, **kw)
        assert np.array_equal(got["out"], want["out"])
        for i, r in enumerate(want["out"]):  # the hit records (target ids and loci) before either side assigns from them
            nh = min(int(r["inst"]), kw["max_ml"]) if r["hit_rslt"] in (1, 2, 3) else 0
            assert np.array_equal(want["hits"][i, :nh], got["hits"][i, :nh]), i
        o_out, o_hits = want["out"].copy(), want["hits"].copy()  # the oracle assigns from its own records
        multi = (o_out["hit_rslt"] == 1) & (o_out["inst"] > 1)
        assert (want["hits"][multi, 1]["chrom_id"] > 128).sum() > 300
        n_want = genomes.oracle.assign_multi_matches(o_out, o_hits, ml_mode, 100, threads=1)
        g_out, g_hits, n_got = ix.assign_multi(got["out"], got["hits"], ml_mode, 100)
        assert n_got == n_want and (g_out == o_out).all()
        acc = g_out["nar"] == 1
        assert (g_hits[acc, 0] == o_hits[acc, 0]).all()
        won = acc & multi
        print("assign multi -r%d: %d reads, %d multi-aligned, %d assigned, %d of them to id > 128" % (ml_mode, len(reads), multi.sum(), n_got,
                                                                                                 _high(g_hits[:, 0], won)))
        assert multi.sum() > 700 and n_got > 100 and _high(g_hits[:, 0], won) > 30
        dup_ids = [t + 1 for pair in mt.DUPLICATES for t in pair]
        assert not np.isin(g_hits[won, 0]["chrom_id"], dup_ids).any()
    finally:
        ix.close()


# ---- SAM and BAM records from these results ------------------------------------------------------------------------------------
def _bam_records(bam):
    """(refID, pos, next_refID, next_pos, read name) of each record of an uncompressed BAM body"""
    recs, off = [], 0
    while off < len(bam):
        size, ref, pos, bmn, _, _, nref, npos, _ = struct.unpack_from("<iiiIIiiii", bam, off)
        recs.append((ref, pos, nref, npos, bam[off + 36:off + 36 + (bmn & 0xFF) - 1].decode()))
        off += 4 + size
    assert off == len(bam)
    return recs


def _check_records(ix, names_c, prep, parsed, names, reads, out=None, hit0=None, pe=None, **dev):
    from test_gpu_io import _sam_lines_host

    body, stats, chrom_hit = ix.format_sam(prep, *parsed, **dev)
    want = _sam_lines_host(names, reads, out, hit0, names_c, pe=pe)
    assert body == want and stats["n_lines"] == want.count(b"\n") > 1000
    ids = pe["hit"]["chrom_id"][pe["nar"] == 1] if pe is not None else hit0["chrom_id"][out["nar"] == 1]
    hit_ids = np.unique(ids)
    assert np.array_equal(np.nonzero(chrom_hit)[0], hit_ids) and (hit_ids > 128).sum() > 50
    rank = {names_c[int(c) - 1]: k for k, c in enumerate(hit_ids)}  # a header of the hit sequences only, in index order
    lines = [l.split("\t") for l in want.decode().splitlines()]
    for sq_all in (False, True):
        bam, bstats, bhit = ix.format_sam(prep, *parsed, bam=True, sq_all=sq_all, **dev)
        assert np.array_equal(bhit, chrom_hit) and bstats["n_lines"] == stats["n_lines"]
        ref_of = (lambda nm: names_c.index(nm)) if sq_all else (lambda nm: rank[nm])
        exp = [(ref_of(f[2]), int(f[3]) - 1, ref_of(f[2]) if f[6] == "=" else -1, int(f[7]) - 1, f[0]) for f in lines]
        assert _bam_records(bam) == exp, sq_all
    return lines


def test_sam_and_bam_records_se_300_targets(k4, genomes, monkeypatch):
    import torch
    from test_gpu_io import _fasta_of

    ix, chroms = _open(k4, genomes, monkeypatch, 300, "el4")
    try:
        names_c = genomes.chroms(300)[0]
        reads = mt.mixed_batch(chroms, 21)
        reads = [r for r in reads if 50 <= len(r) <= 500]
        p1 = ix.parse_fastx(_fasta_of(reads, "se"))
        prep = ix.prepare_reads(p1, min_len=50, max_len=500)
        n = prep["n_units"]
        assert n == len(reads)
        rr = torch.zeros((n, 6), dtype=torch.int32, device=prep["reads"].device)
        hits = torch.zeros((n, 4), dtype=torch.int32, device=prep["reads"].device)
        kp = k4.KalignParams(2, 1, 1, 0, k4.STRAND_BOTH, 1, 0, 0, 0)
        ix.reserve(n, prep["max_len"], 1)
        ix.kalign_batch_dev(kp, n, prep["max_len"], prep["reads"].data_ptr(), prep["offs"].data_ptr(), prep["lens"].data_ptr(), rr.data_ptr(),
                            hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
        want = genomes.want((300, "sam se"), lambda h: genomes.oracle.kalign_batch(h, reads, max_subs=2, threads=8))
        names = ["se%06d" % (i + 1) for i in range(n)]
        _check_records(ix, names_c, prep, (p1,), names, reads, out=want["out"], hit0=want["hits"][:, 0], rr=rr, hits=hits, max_ml=1)
    finally:
        ix.close()


@pytest.mark.parametrize("pe_mode", [1, 3])
def test_sam_and_bam_records_pe_300_targets(k4, genomes, monkeypatch, pe_mode):
    import torch
    from test_gpu_io import _fasta_of

    ix, chroms = _open(k4, genomes, monkeypatch, 300, "el4")
    try:
        names_c = genomes.chroms(300)[0]
        pe1, pe2, kind, _ = mt.pe_batch(chroms, 2500)
        p1, p2 = ix.parse_fastx(_fasta_of(pe1, "a")), ix.parse_fastx(_fasta_of(pe2, "b"))
        prep = ix.prepare_reads(p1, p2, min_len=50, max_len=500)
        n = prep["n_units"]
        d_out = torch.zeros(2 * n * k4.PE_READ_DTYPE.itemsize, dtype=torch.uint8, device=prep["reads"].device)
        kp = k4.KalignParams(2, 1, 1, 0, k4.STRAND_BOTH, 10, 1, 0, 0)
        pp = k4.PeParams(pe_mode, 150, 500, 0)
        ix.kalign_pe_batch_dev(kp, pp, n, prep["max_len"], prep["reads"].data_ptr(), prep["offs"].data_ptr(), prep["lens"].data_ptr(),
                               d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        want = genomes.want((300, "pe", pe_mode), lambda h: oracle_kalign_pe(genomes.oracle, h, pe1, pe2, threads=8, pe_mode=pe_mode,
                                                                             pair_min_len=150, pair_max_len=500, max_subs=2))
        inter = [x for pair in zip(pe1, pe2) for x in pair]
        names = [("a%06d" if i % 2 == 0 else "b%06d") % (i // 2 + 1) for i in range(2 * n)]
        lines = _check_records(ix, names_c, prep, (p1, p2), names, inter, pe=want, pe_recs=d_out)
        # pairs whose ends lie on different targets are reported (`-U3`: each end on its own, without a mate reference)
        by_name = {}
        for f in lines:
            by_name.setdefault(f[0][1:], []).append(f)
        cross = [v for v in by_name.values() if len(v) == 2 and v[0][2] != v[1][2]]
        assert len(cross) > (200 if pe_mode == 3 else -1) and all(f[6] == "*" for v in cross for f in v)
    finally:
        ix.close()


# ---- k4index and k4align end to end against what the reference wrote on the 300-target genome ----------------------------------

@pytest.fixture(scope="module")
def mt300_sfx(tmp_path_factory):
    """The 300-target FASTA through `k4index`, checked against the SHA-256 digests recorded of the file `ngskit4b index` wrote: the
    same length, every part of the file but the suffix array the reference's byte for byte, and the suffix array the reference's once
    the suffixes that compare equal are put in offset order.  (The reference's comparison returns 0 for suffixes identical through
    their first EOS -- byte-identical targets, and every suffix that starts at an EOS, so every index of many targets has them --
    and the order its multithreaded quicksort leaves them in follows no rule: the whole-file SHA-256, recorded too, cannot be
    asserted.)"""
    import synth

    d = tmp_path_factory.mktemp("mt300")
    names, chroms = mt.genome(300)
    fa, sfx = str(d / "mt300.fa"), str(d / "mt300.sfx")
    synth.write_fasta(fa, chroms, names=names)
    p = subprocess.run([os.path.join(ROOT, "kit4b_amd", "k4index"), "-i", fa, "-o", sfx, "-r", "mt300"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "6 sequences not accepted" in p.stderr  # the targets of 1, 7 and 40 bases, as the reference: 294 targets are left
    raw = open(sfx, "rb").read()
    assert len(raw) == MT300["sfx_bytes"]
    parts = mt.sfx_parts(raw)
    for k, v in MT300["sfx_parts_sha256"].items():
        if k != "sa":
            assert parts[k] == v, k
    return sfx


def test_k4index_writes_the_reference_index_up_to_tied_suffixes_300_targets(mt300_sfx):
    """What holds of the file `k4index` writes against the one `ngskit4b index` wrote (the fixture asserts the first two): all parts
    but the suffix array are identical; the suffix array is identical once tied suffixes are in offset order; and `k4index`'s own
    array IS in that form: its order among ties is by offset."""
    parts = mt.sfx_parts(open(mt300_sfx, "rb").read())
    want = MT300["sfx_parts_sha256"]
    assert {k: v for k, v in parts.items() if k != "sa"} == {k: v for k, v in want.items() if k != "sa"}
    assert parts["sa"] == parts["sa_ties_by_offset"] == want["sa_ties_by_offset"]


def _unxz_to(tmp_path, name):
    dst = str(tmp_path / name[:-3])
    open(dst, "wb").write(lzma.open(os.path.join(GOLDEN, name)).read())
    return dst


def _k4align(tmp_path, sfx, case, out, *extra):
    files = []
    for flag, r in zip(("-i", "-u"), MT300["cases"][case]["reads"]):
        files += [flag, _unxz_to(tmp_path, r)]
    p = subprocess.run([os.path.join(ROOT, "kit4b_amd", "k4align"), "-I", sfx, "-o", out] + MT300["cases"][case]["args"] + list(extra) + files,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


def _golden_sam(case):
    lines = lzma.open(os.path.join(GOLDEN, "mt300_%s.sam.xz" % case)).read().decode().splitlines()
    return [l for l in lines if l.startswith("@") and not l.startswith("@PG")], [l for l in lines if not l.startswith("@")]


@pytest.mark.parametrize("case", sorted(MT300["cases"]))
def test_k4align_writes_the_reference_sam_300_targets(mt300_sfx, tmp_path, case):
    """identical header (but @PG: with `-4 100` only the sequences with alignments are declared) and identical records"""
    out = str(tmp_path / "out.sam")
    p = _k4align(tmp_path, mt300_sfx, case, out)
    hdr, recs = _golden_sam(case)
    got = open(out).read().splitlines()
    got_hdr = [l for l in got if l.startswith("@") and not l.startswith("@PG")]
    got_recs = [l for l in got if not l.startswith("@")]
    n_sq = sum(l.startswith("@SQ") for l in got_hdr)
    assert n_sq == MT300["cases"][case]["n_sq"] and (100 < n_sq < 294 if "-4" in MT300["cases"][case]["args"] else n_sq == 294)
    assert got_hdr == hdr
    assert sorted(got_recs) == sorted(recs)
    order = {l.split("\tSN:")[1].split("\t")[0]: i for i, l in enumerate(h for h in hdr if h.startswith("@SQ"))}
    aligned = [l.split("\t") for l in got_recs if l.split("\t")[2] != "*"]
    keys = [(order[f[2]], int(f[3])) for f in aligned]
    assert keys == sorted(keys) and sum(int(f[2][1:]) > 128 for f in aligned) > 500  # (target names: "t" + the index in the FASTA + 1)
    if "-r5" in MT300["cases"][case]["args"]:  # the reference tallies reported loci, not reads, in this mode
        assert ("%d alignments written" % MT300["cases"][case]["nar"]["AA"]) in p.stderr
        return
    for name, n in MT300["cases"][case]["nar"].items():
        assert ("%d (%s)" % (n, name)) in p.stderr, (name, n)


@pytest.mark.parametrize("case", ["se_s2_sq100", "pe_u2_sq100"])
def test_k4align_bam_of_the_hit_sequences_only(mt300_sfx, tmp_path, case):
    """`-4 100 -o out.bam`: the dictionary is the SAM's @SQ list, in its order, refIDs number that list, and the .bai answers region
    queries by those refIDs"""
    import random

    import samutil
    from test_bam_cpu import brute, regions

    out = str(tmp_path / "out.bam")
    _k4align(tmp_path, mt300_sfx, case, out)
    hdr, recs = _golden_sam(case)
    text, refs, brecs, blocks = samutil.read_bam(out, with_offsets=True)
    sq = [(l.split("\tSN:")[1].split("\t")[0], int(l.split("\tLN:")[1].split("\t")[0])) for l in hdr if l.startswith("@SQ")]
    assert [(r[0], r[1]) for r in refs] == sq and len(sq) == MT300["cases"][case]["n_sq"] < 294
    assert [l for l in text.splitlines() if not l.startswith("@PG")] == hdr
    assert sorted(samutil.bam_record_as_sam_fields(r, refs) for r in brecs) == sorted(samutil.sam_line_fields(l) for l in recs)
    assert [(r["ref"], r["pos"]) for r in brecs] == sorted((r["ref"], r["pos"]) for r in brecs)
    bai = samutil.read_bai(out + ".bai")
    rng = random.Random(300)
    for ref, beg, end in regions(refs, rng, 80):
        assert samutil.bai_fetch(brecs, blocks, bai, ref, beg, end) == brute(brecs, ref, beg, end)


@pytest.mark.parametrize("case", ["se_s2_sq100", "pe_u2_sq100"])
def test_k4align_shards_merge_to_the_reference_sam_300_targets(mt300_sfx, tmp_path, case):
    """`-S 0/2` + `-S 1/2` under `-4 100`, then `k4merge -4 100`: the merged header declares the sequences that received a record in any
    shard -- the single run's header -- and the records are the single run's"""
    shards = []
    for k in range(2):
        o = str(tmp_path / ("s%d.sam" % k))
        _k4align(tmp_path, mt300_sfx, case, o, "-S", "%d/2" % k)
        shards.append(o)
    sqs = [[l for l in open(o).read().splitlines() if l.startswith("@SQ")] for o in shards]
    merged = str(tmp_path / "m.sam")
    p = subprocess.run([os.path.join(ROOT, "kit4b_amd", "k4merge"), "-4", "100", merged] + shards, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    hdr, recs = _golden_sam(case)
    got = open(merged).read().splitlines()
    assert [l for l in got if l.startswith("@") and not l.startswith("@PG")] == hdr
    assert sorted(l for l in got if not l.startswith("@")) == sorted(recs)
    want_sq = [l for l in hdr if l.startswith("@SQ")]
    assert len(want_sq) < 294 and all(len(s) == 294 for s in sqs)  # (a shard declares every sequence and leaves the rule to the merge)
    # without the shards' `-4` the merge applies kalign's default of 10 000 and keeps all 294
    p = subprocess.run([os.path.join(ROOT, "kit4b_amd", "k4merge"), merged] + shards, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and sum(l.startswith("@SQ") for l in open(merged).read().splitlines()) == 294
