"""tests/bigbatch.py without a GPU: the tiled batch and the gather give what a batch of copied reads gives, and the slot model of
the step kernels' survivor and deferred lists stays inside the buffers k4_reserve sets aside -- for every shape
tests/test_gpu_bigbatch.py sends and over a sweep of batch sizes and of survivor / deferred shares."""
import os
import re

import numpy as np
import pytest

import bigbatch as bb
import synth

G = bb.G
ALIGN_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kit4b_amd", "csrc", "k4_align.hip")


def k4_survivor_slots(cap):
    """k4_survivor_slots, kit4b_amd/csrc/k4_align.hip: `return cap + cap / 7 + (size_t)2 * 2048 * 4 * K4_CHUNK + K4_CHUNK;`"""
    return cap + cap // 7 + 2 * 2048 * 4 * 512 + 512


def one_launch_bound(cap):
    """the bound before the split first launch was counted: one partly used chunk per wave of the grid"""
    return cap + cap // 7 + 2048 * 4 * 512 + 512


def test_formula_is_the_one_in_the_source():
    src = open(ALIGN_HIP).read()
    body = re.search(r"static size_t k4_survivor_slots\(size_t cap\) \{(.*?)\n\}", src, re.S).group(1)
    assert "return cap + cap / 7 + (size_t)2 * 2048 * 4 * K4_CHUNK + K4_CHUNK;" in body
    assert re.search(r"#define K4_CHUNK 512\b", open(os.path.join(os.path.dirname(ALIGN_HIP), "k4_align_common.h")).read())
    for cap in (256, 528640, 4980736):
        assert bb.survivor_slots(cap) == k4_survivor_slots(cap)
    assert bb.reserved_slots(G + 4097) == k4_survivor_slots(528640)


# ---- tiling and gather ---------------------------------------------------------------------------------------------------------
def test_tile_names_every_pool_read_m_times():
    pool = [np.full(5 + i % 7, i % 4, dtype=np.uint8) for i in range(300)]
    (cat, offs, lens), idx = bb.tile(pool, 5, seed=3, tail=17)
    assert cat.dtype == np.uint8 and offs.dtype == np.uint64 and lens.dtype == np.uint32
    assert len(cat) == sum(len(r) for r in pool) and len(idx) == 5 * 300 + 17
    assert np.array_equal(np.bincount(idx), np.where(np.arange(300) < 17, 6, 5))
    assert not np.array_equal(idx[:300], np.arange(300))  # permuted
    assert np.array_equal(bb.tile(pool, 5, seed=3, tail=17)[1], idx) and not np.array_equal(bb.tile(pool, 5, seed=4, tail=17)[1], idx)
    for j in (0, 299, 1516):
        assert np.array_equal(cat[int(offs[j]):int(offs[j]) + int(lens[j])], pool[idx[j]])


def test_tiled_batch_equals_copied_reads_through_the_oracle(oracle, golden_dir):
    ho = oracle.open(os.path.join(golden_dir, "g1.sfx"))
    try:
        oracle.set_max_iter(ho, 5000)
        chroms = synth.golden_genome()[1]
        pool, _ = synth.make_reads(chroms[:3], 200, 100, seed=11, sub_lambda=2.0, n_prob=0.05, edge_frac=0.05, random_frac=0.03)
        tiled, idx = bb.tile(pool, 3, seed=5)
        copied = [pool[i].copy() for i in idx]
        kw = dict(max_subs=5, max_ml=10, pe_mode=1)
        raw = (4, 20, 20, 30, 0, 1, 0, 3)
        for run, mh in ((lambda r: oracle.kalign_batch(ho, r, threads=4, **kw), 10),
                        (lambda r: oracle.align_reads_batch(ho, r, *raw, threads=4), 3)):
            a, b, p = run(tiled), run(copied), run(pool)
            e = bb.expect(p, idx)
            for k in b:
                if k != "counters":
                    assert np.array_equal(a[k], b[k]) and np.array_equal(e[k], b[k]), k
            assert a["counters"] == b["counters"] == {k: 3 * v for k, v in p["counters"].items()}
            bb.same(a, e, mh, "tiled")
            bb.same(b, e, mh, "copied", idx)
    finally:
        oracle.close(ho)


# ---- the slot model ------------------------------------------------------------------------------------------------------------
def test_model_grid_and_chunks_by_hand():
    m = bb.slot_model(1000, 4, 64)           # 4 blocks of 256: 16 waves, the last holds 40 reads
    assert (m["grid_blocks"], m["waves"], m["passes"], m["out_slots"], m["survivors"]) == (4, 16, 1, 16 * 512, 1000)
    m = bb.slot_model(G + 4097, 16, 64)      # 4096 blocks of 128; 65 waves take a second read per lane, the last of them one read
    assert (m["grid_blocks"], m["waves"], m["passes"], m["out_slots"], m["survivors"]) == (4096, 8192, 2, 8192 * 512, G + 4097)
    assert bb.slot_model(G + 4097, 4, 0)["out_slots"] == 0
    # nine passes of 61 survivors: eight fill 488 slots, the ninth does not fit the 24 left -> they are retired, a second chunk
    m = bb.slot_model(9 * G, 4, 61)
    assert m["passes"] == 9 and m["out_slots"] == 2 * 8192 * 512 and m["survivors"] == 9 * 61 * 8192
    assert bb.slot_model(8 * G, 4, 61)["out_slots"] == 8192 * 512  # eight passes: one chunk per wave, untouched tail only
    m = bb.slot_model(19 * G // 2, 4, 61)    # half the waves run a tenth pass
    assert m["passes"] == 10 and m["out_slots"] == 2 * 8192 * 512 and m["survivors"] == (9 * 8192 + 4096) * 61
    # split first launch, 32 of 64 set aside: 8192 deferred chunks of 32.  The stride is a multiple of K4_CHUNK, so a wave of the
    # second launch meets the same 64-slot segment of every chunk it walks: only the waves on segment 0 (one in eight) find entries
    m = bb.slot_model(G, 4, 64, 32)
    assert (m["defer_slots"], m["deferred"], m["out_slots"], m["survivors"]) == (8192 * 512, G // 2, (8192 + 1024) * 512, G)
    # 9.5 passes of 58 set aside: a chunk of 464 (the ninth 58 does not fit the 48 left) and a second one per wave; the second
    # launch walks 16384 chunks, retired tails included
    m = bb.slot_model(19 * G // 2, 4, 64, 58)
    assert (m["defer_slots"], m["deferred"]) == (2 * 8192 * 512, (9 * 8192 + 4096) * 58) and m["survivors"] == 19 * G // 2


def test_split_first_launch_needs_two_chunks_per_wave():
    """The bound argued for one launch (one partly used chunk per wave of the grid) does not cover step 0 of a split first launch:
    both launches append to one list and each wave can leave a partly used chunk in either.  The worst placement -- an upper
    bound, whatever the order of the atomics -- passes the earlier bound; evenly placed survivors come within 5 % of it."""
    for n, s, d in ((G, 64, 32), (G + 4097, 64, 58), (19 * G // 2, 64, 58)):
        w = bb.slot_model(n, 4, s, d, placement="worst")
        assert w["out_slots"] > one_launch_bound((n + 255) // 256 * 256), (n, w)
        assert w["out_slots"] <= bb.reserved_slots(n) and w["defer_slots"] <= bb.reserved_slots(n), (n, w)
    e = bb.slot_model(19 * G // 2, 4, 64, 58)
    assert 0.95 * one_launch_bound(19 * G // 2) < e["out_slots"] <= one_launch_bound(19 * G // 2)
    assert bb.slot_model(60000, 4, 64, 32, placement="worst")["out_slots"] <= one_launch_bound(60160)  # (the largest batch of the earlier tests)


# every batch tests/test_gpu_bigbatch.py sends: (case, n, length class, first launch split)
GPU_SHAPES = [("a", G + 4097, 4, False), ("a", G + 4097, 5, False), ("a", G + 4097, 8, False), ("a", G + 4097, 16, False),
              ("b", 19 * G // 2, 4, False), ("c", G + 4097, 4, True), ("c", 19 * G // 2, 4, True), ("d", 40960, 16, False),
              ("d tandem", 1024, 4, True), ("e", 70, 4, False)]


@pytest.mark.parametrize("case,n,nch,split", GPU_SHAPES)
def test_gpu_shapes_stay_inside_the_survivor_buffers(case, n, nch, split):
    """both lists (the deferred one lives in ids[1], a buffer of the same size), whatever share survives or is set aside"""
    assert bb.fits(n, nch, split)
    cap = (n + 255) // 256 * 256
    for d in (bb.SHARES if split else (None,)):
        for s in bb.SHARES:
            for placement in ("even", "worst") if n <= 19 * G // 2 and s in (0.5, 0.95, 1) and d in (None, 0.5, 0.95) else ("worst",):
                m = bb.slot_model(n, nch, 64 * s, None if d is None else 64 * d, placement=placement)
                assert m["out_slots"] <= k4_survivor_slots(cap) and m["defer_slots"] <= k4_survivor_slots(cap), (s, d, placement, m)


def test_even_placement_never_exceeds_the_worst():
    for n in (G + 4097, 3 * G + 77):
        for s in (3, 32, 61, 64):
            for d in (None, 3, 32, 58):
                e, w = bb.slot_model(n, 4, s, d), bb.slot_model(n, 4, s, d, placement="worst")
                assert e["out_slots"] <= w["out_slots"] and e["defer_slots"] <= w["defer_slots"], (n, s, d, e, w)


def sweep():
    """worst ratio of used to reserved slots over n = G .. 32 M (40 steps, both block sizes) and the shares of survivors and of
    deferred reads; with the shape that has it"""
    worst = (0.0, None)
    sizes = sorted({int(v) for v in np.geomspace(G, 32 * 2 ** 20, 40)} | {G, G + 4097, 19 * G // 2})
    for n in sizes:
        reserved = bb.reserved_slots(n)
        for nch in (4, 16):
            for d in (None,) + bb.SHARES:
                for s in bb.SHARES:
                    m = bb.slot_model(n, nch, 64 * s, None if d is None else 64 * d, placement="worst")
                    nxt = bb.later_step_slots(m["out_slots"], m["survivors"], n, nch, 64)
                    r = max(m["out_slots"], m["defer_slots"], nxt) / reserved
                    if r > worst[0]:
                        worst = (r, (n, nch, d, s))
    return worst


def test_sweep_of_legal_shapes_stays_inside_the_survivor_buffers():
    ratio, shape = sweep()
    print("worst used / reserved slots: %.4f at (n, nch, deferred share, survivor share) = %s" % (ratio, shape))
    assert ratio <= 1.0, (ratio, shape)
    assert ratio > 0.9  # (and the model is no idle bound: the split launch of one full grid comes close)
