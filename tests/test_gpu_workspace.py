"""The device memory an index owns (k4_internal.h: the K4DevBuf members of k4_index / K4Workspace): every grow path of the
workspace, of the host-pointer staging, of the paired-end pass and of the mate-rescue staging on one handle, then the closing
of that handle -- each call compared with the CPU oracle, field for field and hit slot for hit slot."""
import ctypes as C
import os

import numpy as np
import pytest

import synth
from oracle_bindings import oracle_kalign_pe
from test_gpu_parity import check_against

pytestmark = pytest.mark.gpu

RESULT_FIELDS = ("hit_rslt", "inst", "low_mm", "nxt_mm", "nar", "num_hits")
PE_FIELDS = ("nar", "num_hits", "inst", "low_mm", "pe_aligned", "rescued")
RESCUE_TASK_DTYPE = np.dtype(  # k4_rescue_task, include/k4sfx.h
    [("chrom_id", "<u4"), ("start_loci", "<u4"), ("end_loci", "<u4"), ("read_len", "<u4"), ("read_off", "<u8"),
     ("b3prime_extend", "<i4"), ("antisense", "<i4"), ("min_insert", "<i4"), ("max_insert", "<i4"), ("max_allowed_mm", "<i4"),
     ("chimeric", "<u4")])


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


@pytest.fixture(scope="module")
def g1(golden_dir):
    return os.path.join(golden_dir, "g1.sfx")


@pytest.fixture(scope="module")
def chroms():
    return synth.golden_genome()[1]


def open_pair(k4, oracle, path):
    ix = k4.SfxIndex.open(path)
    ho = oracle.open(path)
    ix.set_max_iter(5000)
    oracle.set_max_iter(ho, 5000)
    return ix, ho


def check_kalign(eg, eo, max_ml, what):
    for f in RESULT_FIELDS:
        bad = np.nonzero(eo["out"][f] != eg["out"][f])[0]
        assert len(bad) == 0, (what, f, bad[:5], eo["out"][f][bad[:5]], eg["out"][f][bad[:5]])
    for i, r in enumerate(eo["out"]):
        nh = min(int(r["inst"]), max_ml) if r["hit_rslt"] in (1, 2, 3) else 0
        assert np.array_equal(eo["hits"][i, :nh], eg["hits"][i, :nh]), (what, i)
        assert not eg["hits"][i, nh:].view(np.uint8).any(), (what, i, "stale hit slots")


def check_pe(g, o, what):
    for f in PE_FIELDS:
        bad = np.nonzero(g[f] != o[f])[0]
        assert len(bad) == 0, (what, f, bad[:6], g[f][bad[:6]], o[f][bad[:6]])
    acc = g["nar"] == 1
    assert acc.sum() > 0 and np.array_equal(g["hit"][acc], o["hit"][acc]), what


def test_se_grow_paths_on_one_handle(k4, oracle, g1, chroms):
    """small pinned block -> first separate staging set (K4_SMALL_READS + 1 reads) -> workspace and staging regrow (5-word rows,
    more reads) -> 16-word rows and four hit slots per read -> the first batch again (nothing regrows) -> LocateBestMatches."""
    ix, ho = open_pair(k4, oracle, g1)
    try:
        raw = dict(tot_mm=1, core_len=18, core_delta=18, max_slides=3, max_hits=2)
        r50 = synth.make_reads(chroms, 3, 50, seed=11, sub_lambda=0.5)[0]
        first = ix.align_reads_batch(r50, **raw)
        exp50 = oracle.align_reads_batch(ho, r50, **raw)
        check_against(first, exp50, raw["max_hits"], "3 x 50")
        for n, rl, kw in ((4097, 100, dict(max_subs=2)), (4200, 150, dict(max_subs=3)), (300, 300, dict(max_subs=2, max_ml=4))):
            reads = synth.make_reads(chroms, n, rl, seed=rl + n, n_prob=0.03, edge_frac=0.05, random_frac=0.03, sub_lambda=1.5)[0]
            check_kalign(ix.kalign_batch(reads, **kw), oracle.kalign_batch(ho, reads, threads=8, **kw), kw.get("max_ml", 1),
                         "%d x %d" % (n, rl))
        again = ix.align_reads_batch(r50, **raw)
        for k in ("rslt", "inst", "low", "nxt", "hits"):
            assert np.array_equal(again[k], first[k]), k
        r5 = synth.make_reads(chroms, 5, 100, seed=8181, sub_lambda=1.6)[0]
        g = ix.best_matches_batch(r5, 3, 25, 25, 8, max_hits=6)
        L = oracle.L
        L.k4o_locate_best_matches.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int),
                                                                             C.c_void_p, C.c_int, C.c_void_p]
        for i, rd in enumerate(r5):
            buf = np.ascontiguousarray(rd, dtype=np.uint8).copy()
            hits = np.zeros(7, dtype=g["hits"].dtype)
            inst = C.c_int(0)
            r = L.k4o_locate_best_matches(ho, 3, 25, 25, 8, 0, buf.ctypes.data, len(buf), 6, C.byref(inst), hits.ctypes.data, 5000, None)
            assert (r, inst.value) == (int(g["rslt"][i]), int(g["inst"][i])), i
            assert np.array_equal(hits[: inst.value], g["hits"][i][: inst.value]), i
            assert not g["hits"][i][inst.value:].view(np.uint8).any()
    finally:
        ix.close()
        oracle.close(ho)


def test_se_ext_batch_with_second_segments(k4, oracle, g3_path, golden_dir):
    """k4_kalign_ext_batch with its k4_seg2 output (the temporary second-segment array, the shared download tail)"""
    g = np.load(os.path.join(golden_dir, "align_ext_all_100.npz"))
    pick = np.linspace(0, len(g["lens"]) - 1, 50).astype(int)
    reads = [g["reads"][int(g["offs"][i]):int(g["offs"][i]) + int(g["lens"][i])] for i in pick]
    ix, ho = open_pair(k4, oracle, g3_path)
    try:
        kw = dict(max_subs=3, min_chimeric_len=50, micro_indel_len=15, max_splice_junct_len=4000)
        a = ix.kalign_ext_batch(reads, **kw)
        b = oracle.kalign_ext_batch(ho, reads, **kw)
        for k in ("out", "hits", "seg2"):
            d = a[k] != b[k]
            if d.ndim > 1:
                d = d.any(axis=1)
            assert not d.any(), (k, np.nonzero(d)[0][:5], a[k][d][:2], b[k][d][:2])
        assert (a["seg2"]["match_len"] > 0).sum() > 0
    finally:
        ix.close()
        oracle.close(ho)


def test_pe_grow_paths_on_one_handle(k4, oracle, g1, chroms):
    """pe_reserve: first allocation, regrowth by pairs, regrowth by hit slots (max(max_ml, 10) per end)"""
    ix, ho = open_pair(k4, oracle, g1)
    try:
        kw = dict(pe_mode=1, pair_min_len=220, pair_max_len=640, pair_strand=False, max_subs=2)
        for n, max_ml in ((200, 10), (1000, 10), (200, 12)):
            pe1, pe2, _ = synth.make_pe_reads(chroms, n, 125, seed=500 + n + max_ml, sub_lambda=1.8, n_prob=0.03, random_mate_frac=0.05,
                                              frag_min=260, frag_max=700)
            g = ix.kalign_pe_batch(pe1, pe2, max_ml=max_ml, **kw)
            check_pe(g, oracle_kalign_pe(oracle, ho, pe1, pe2, threads=8, **kw), (n, max_ml))
    finally:
        ix.close()
        oracle.close(ho)


def rescue_tasks(chroms, n, read_len, seed):
    """n AlignPairedRead calls on made-up anchors: windows below and above 1000 loci, both sides, both strands; most mates lie
    inside their window with a few substitutions, some are random sequence"""
    rng = np.random.default_rng(seed)
    tasks = np.zeros(n, dtype=RESCUE_TASK_DTYPE)
    reads = []
    for t in range(n):
        c = int(rng.integers(0, 3))
        g = chroms[c]
        window = int(rng.choice([400, 900, 1500]))
        b3 = bool(rng.integers(0, 2))
        a_start = int(rng.integers(window + read_len + 100, len(g) - window - read_len - 200))
        a_end = a_start + 99
        frag = int(rng.integers(read_len + 20, window))
        m_start = (a_start + frag - read_len) if b3 else (a_end - frag + 1)
        mate = g[m_start:m_start + read_len].copy()
        for _ in range(int(rng.integers(0, 5))):
            p = int(rng.integers(3, read_len - 3))
            mate[p] = (mate[p] + 1 + rng.integers(0, 3)) % 4
        if rng.random() < 0.1:
            mate = rng.integers(0, 4, read_len).astype(np.uint8)  # nothing to find
        anti = bool(rng.integers(0, 2))
        if anti:
            mate = (3 - mate)[::-1].copy()
        tasks[t] = (c + 1, a_start, a_end, read_len, t * read_len, int(b3), int(anti), 50, window + read_len, int(rng.choice([2, 3, 5])), 0)
        reads.append(mate)
    return tasks, np.ascontiguousarray(np.concatenate(reads), dtype=np.uint8)


def test_mate_rescue_staging_grows(k4, oracle, g1, chroms):
    """k4_mate_rescue_batch: the staging at its floors (256 tasks, 64 KiB of reads), then above both"""
    ix, ho = open_pair(k4, oracle, g1)
    L = oracle.L
    L.k4o_align_paired_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p, C.c_void_p]
    try:
        for n in (10, 300):
            tasks, cat = rescue_tasks(chroms, n, 250, seed=40 + n)
            assert n <= 256 or len(cat) > (1 << 16)
            rslt = np.full(n, -99, dtype=np.int32)
            hits = np.zeros(n, dtype=k4.HIT_DTYPE)
            ix._ck(k4.lib().k4_mate_rescue_batch(ix.h, n, tasks.ctypes.data, cat.ctypes.data, len(cat), rslt.ctypes.data, hits.ctypes.data))
            for t, tk in enumerate(tasks):
                rd = cat[int(tk["read_off"]):int(tk["read_off"]) + 250].copy()
                h = np.zeros(1, dtype=k4.HIT_DTYPE)
                r = L.k4o_align_paired_read(ho, int(tk["b3prime_extend"]), int(tk["antisense"]), int(tk["chrom_id"]), int(tk["start_loci"]),
                                            int(tk["end_loci"]), int(tk["min_insert"]), int(tk["max_insert"]), int(tk["max_allowed_mm"]),
                                            250, rd.ctypes.data, h.ctypes.data)
                assert r == rslt[t], (n, t, r, rslt[t])
                if r == 1:
                    assert h[0].tobytes() == hits[t].tobytes(), (n, t, h[0], hits[t])
                else:
                    assert not hits[t:t + 1].view(np.uint8).any(), (n, t)
        assert (rslt == 1).sum() > 100 and (rslt == 0).sum() > 10  # (the 300 tasks: placed mates and mates with no placement)
    finally:
        ix.close()
        oracle.close(ho)


def test_close_of_an_unused_handle_and_after_a_refused_call(k4, oracle, g1, chroms):
    """open / close with no workspace at all; open, one refused call, close; the device is fit for use afterwards"""
    import torch

    k4.SfxIndex.open(g1).close()
    ix = k4.SfxIndex.open(g1)
    r50 = synth.make_reads(chroms, 3, 50, seed=11, sub_lambda=0.5)[0]
    with pytest.raises(k4.K4Error):
        ix.align_reads_batch(r50, 1, 0, 18, 3)  # core_len 0
    ix.close()
    torch.cuda.synchronize()  # (raises on a pending device error)
    ix, ho = open_pair(k4, oracle, g1)
    try:
        raw = dict(tot_mm=1, core_len=18, core_delta=18, max_slides=3, max_hits=2)
        check_against(ix.align_reads_batch(r50, **raw), oracle.align_reads_batch(ho, r50, **raw), 2, "after reopen")
    finally:
        ix.close()
        oracle.close(ho)
