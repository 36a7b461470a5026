"""Lean survivor rows and tile claims of the step kernels (-m gpu), read for read against the CPU oracle: records, hit slots and
the tallies n_lookup / n_cand.

 a. the reverse-complement column a later phase rebuilds from the forward words: reads with 0, 1 and 2 substitutions on both
    strands at lengths on either side of every word boundary and at both ends of every length class, `-s2` so that the second
    and the third phase run; survivors with a memo (empty or single-suffix offset-0 bucket) and without one
 b. four lengths in one batch of one class: the length in the survivor's slot is the read's own
 c. tile claims: n no multiple of the tile or of 64, n smaller than one tile, n past one tile for every wave of the largest grid
    (at least one wave claims twice), and a split first launch (both of its claim counters) on the repeat-family index"""
import numpy as np
import pytest

import bigbatch as bb
import synth
from test_gpu_bigbatch import family, g1, k4  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

S2 = dict(max_subs=2, max_ml=1)
TILE = 256               # K4_TILE_GROUPS * 64, k4_align_common.h
MAX_WAVES = 2048 * 4     # the largest grid of a step kernel (k4_resident_blocks, k4_align.hip)
CLASSES = {4: (31, 32, 33, 63, 64, 65, 100, 127, 128), 5: (129, 160), 8: (161, 256), 16: (257, 512)}


def planted(chroms, rl, per_subs, seed):
    """per_subs reads each with 0, 1 and 2 substitutions, either strand, no N"""
    reads = []
    for subs in (0, 1, 2):
        reads += synth.make_reads(chroms[:3], per_subs, rl, seed=seed + subs, fixed_subs=subs)[0]
    return [r for r in reads if r.max() <= 3]


def check(ix, oracle, ho, reads, what, kw=S2, batch=None, pool_idx=None, times=1):
    """the batch (the reads themselves, or `batch` = the reads tiled `times` times) against the oracle's result for the reads"""
    po = oracle.kalign_batch(ho, reads, threads=8, **kw)
    ix.reset_counters()
    got = ix.kalign_batch(reads if batch is None else batch, **kw)
    want = po if pool_idx is None else bb.expect(po, pool_idx)
    bb.same(got, want, kw["max_ml"], what, pool_idx)
    c = ix.counters()
    n = len(reads) * times
    assert c["n_reads"] == n, (what, c)
    assert c["n_lookup"] == times * po["counters"]["n_lookup"] and c["n_cand"] == times * po["counters"]["n_cand"], (what, c, po["counters"])
    return po


@pytest.mark.parametrize("nch", sorted(CLASSES))
def test_rebuilt_reverse_complement(k4, oracle, g1, nch):
    ix, ho, chroms = g1
    k = ix.info()["kmer_k"]
    counts = bb.kmer_counts(chroms, k)
    reads = []
    for rl in CLASSES[nch]:
        reads += planted(chroms, rl, 100, seed=rl * 7)
    assert max(len(r) for r in reads) == max(CLASSES[nch]) and len(reads) >= 270 * len(CLASSES[nch])
    po = check(ix, oracle, ho, reads, ("rebuilt reverse complement", nch))
    o = po["out"]
    # hits on the '-' strand found behind the first phase: through the rebuilt column
    later = np.isin(o["hit_rslt"], (1, 2, 3)) & (o["low_mm"] >= 1)
    strands = po["hits"]["strand"][:, 0]
    assert (later & (strands == ord("-"))).sum() >= 20 * len(CLASSES[nch]) and (later & (strands == ord("+"))).sum() >= 20 * len(CLASSES[nch])
    assert set(o["low_mm"][later].tolist()) >= {1, 2}  # the second and the third phase both settle reads
    # survivors of the first phase whose '+' pass met an empty, a single-suffix and a deeper offset-0 bucket: memo kinds 1, 2, none
    depth = np.array([counts[bb.kmer_code(r, k)] for r in reads])
    survivors = ~(np.isin(o["hit_rslt"], (1, 2, 3)) & (o["low_mm"] == 0))
    assert (survivors & (depth == 0)).any() and (survivors & (depth == 1)).any() and (survivors & (depth >= 2)).any()


def test_mixed_lengths_in_one_batch(k4, oracle, g1):
    ix, ho, chroms = g1
    per_len = [planted(chroms, rl, 100, seed=rl * 11) for rl in (40, 77, 100, 128)]
    reads = [r for quad in zip(*per_len) for r in quad]  # neighbouring lanes hold different lengths
    assert len(reads) >= 1000 and [len(r) for r in reads[:4]] == [40, 77, 100, 128]
    po = check(ix, oracle, ho, reads, "mixed lengths")
    o = po["out"]
    lens = np.array([len(r) for r in reads])
    for rl in (40, 77, 100, 128):  # every length has reads that a later phase settles
        assert (np.isin(o["hit_rslt"], (1, 2, 3)) & (o["low_mm"] >= 1) & (lens == rl)).sum() >= 50, rl


@pytest.fixture(scope="module")
def pool100(g1):
    _, _, chroms = g1
    pool = planted(chroms, 100, 1400, seed=9100)[:4093]
    assert len(pool) == 4093
    return pool


@pytest.mark.parametrize("n", [70, 200, 4 * TILE + 13 + 64])
def test_tile_claims_small_batches(k4, oracle, g1, pool100, n):
    ix, ho, _ = g1
    assert n % 64 and n % TILE and (n < TILE or n > 4 * TILE)
    check(ix, oracle, ho, pool100[:n], ("tile claims", n))


def test_tile_claims_a_wave_claims_twice(k4, oracle, g1, pool100):
    ix, ho, _ = g1
    m = 513
    n = m * len(pool100)
    assert n > MAX_WAVES * TILE and n - MAX_WAVES * TILE < 4096 and n % 64 and n % TILE  # more tiles than any grid has waves
    assert bb.fits(n, 4, False)
    batch, idx = bb.tile(pool100, m, seed=513)
    check(ix, oracle, ho, pool100, ("tile claims", n), batch=batch, pool_idx=idx, times=m)


def test_tile_claims_split_first_launch(k4, oracle, family):
    ix, ho, chroms, counts, k, pool = family
    deep = counts > bb.K4_DEEP_BUCKET
    assert counts[deep].sum() / counts.sum() >= 10 * bb.K4_DEFER_MIN_FRAC  # the first launch is split on this index
    pool = pool[:4093]
    m = 3
    n = m * len(pool)
    assert n % 64 and n % TILE and n > 16 * TILE and bb.fits(n, 4, True)
    set_aside = np.array([counts[bb.kmer_code(r, k)] > bb.K4_DEEP_BUCKET for r in pool])
    assert set_aside.mean() >= 0.85  # the second launch's list is longer than a tile, the first launch leaves survivors too
    batch, idx = bb.tile(pool, m, seed=3)
    check(ix, oracle, ho, pool, ("split first launch", n), kw=dict(max_subs=5, max_ml=1), batch=batch, pool_idx=idx, times=m)
