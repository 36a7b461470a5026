"""The step kernels and the general kernel at batch sizes where grids stride and chunks roll (-m gpu): batches of up to 5 M reads,
tiled from a pool of at most 4096 that goes through the CPU oracle once (tests/bigbatch.py), every read compared.

 a. n = G + 4097: lanes take a second read in step 0 while the last wave is partly filled; every length class
 b. n = 9.5 G, most reads surviving: a wave passes 512 survivors, retires the tail of its chunk and rolls over
 c. the same sizes on an index whose first launch is split: the deferred list, walked by the second launch
 d. a slow list longer than K4_SLOW_WAVES and a huge list longer than K4_HUGE_WAVES
 e. batches of 5 M, 0.5 M and 70 reads on one handle
G = 524288 lanes is one full grid of every length class."""
import ctypes as C
import os

import numpy as np
import pytest

import bigbatch as bb
import synth
from test_gpu_step_plan import RAW_SETS

pytestmark = pytest.mark.gpu

G = bb.G
N_SECOND_PASS = G + 4097
N_ROLLOVER = 19 * G // 2
KALIGN = (dict(max_subs=5, max_ml=1), dict(max_subs=5, max_ml=10, pe_mode=1))


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


@pytest.fixture(scope="module")
def g1(k4, oracle, golden_dir):
    path = os.path.join(golden_dir, "g1.sfx")
    ix = k4.SfxIndex.open(path)
    ho = oracle.open(path)
    ix.set_max_iter(5000)
    oracle.set_max_iter(ho, 5000)
    yield ix, ho, synth.golden_genome()[1]
    ix.close()
    oracle.close(ho)


def index_from_oracle(k4, oracle, names, chroms):
    """the oracle's suffix array under the GPU index, as test_deep_repeats_vs_oracle builds it"""
    ho = oracle.build(names, chroms, threads=8)
    n = oracle.concat_len(ho)
    sa_raw = np.ctypeslib.as_array(C.cast(oracle.L.k4o_sa_bytes(ho), C.POINTER(C.c_uint8)), shape=(n * 4,))
    ix = k4.SfxIndex.from_host(np.array(oracle.seq(ho)), sa_raw, 4, k4.make_entries(names, [len(c) for c in chroms]))
    oracle.set_max_iter(ho, 5000)
    ix.set_max_iter(5000)
    return ix, ho


def run_tiled(ix, pool_result, batch, pool_idx, max_hits, what, call):
    """one tiled batch through the public host entry, every read against the pool's oracle result"""
    got = call(batch)
    bb.same(got, bb.expect(pool_result, pool_idx), max_hits, what, pool_idx)
    return got


def batch_of(pool, n, seed):
    return bb.tile(pool, n // len(pool), seed, tail=n % len(pool))


# ---- a. second grid pass, every length class -----------------------------------------------------------------------------------
def class_pool(chroms, rl):
    """about 3600 reads of rl bases with 0..6 substitutions, reads at the ends of the entries among them"""
    pool = []
    for subs in range(7):
        pool += synth.make_reads(chroms[:3], 500, rl, seed=rl * 10 + subs, fixed_subs=subs, edge_frac=0.03)[0]
    pool += synth.make_reads(chroms[:3], 100, rl, seed=rl * 10 + 9, sub_lambda=1.0, edge_frac=1.0)[0]
    return pool


@pytest.mark.parametrize("rl,nch", [(100, 4), (150, 5), (250, 8), (400, 16)])
def test_second_grid_pass(k4, oracle, g1, rl, nch):
    ix, ho, chroms = g1
    n = N_SECOND_PASS
    assert n > G and n % G < 64 * 128 and (n % 64) != 0  # a second pass for a few waves only, the last of them partly filled
    assert bb.slot_model(n, nch, 64)["passes"] == 2 and bb.fits(n, nch, False)
    pool = class_pool(chroms, rl)
    assert len(pool) <= 4096 and {4: rl <= 128, 5: 128 < rl <= 160, 8: 160 < rl <= 256, 16: 256 < rl <= 512}[nch]  # nch_for, k4_align.hip
    batch, idx = batch_of(pool, n, seed=rl)
    assert len(idx) == n and np.bincount(idx).min() == n // len(pool)
    kw = KALIGN[0]
    run_tiled(ix, oracle.kalign_batch(ho, pool, threads=8, **kw), batch, idx, 1, ("second pass kalign", rl),
              lambda b: ix.kalign_batch(b, **kw))
    p = RAW_SETS[0]
    run_tiled(ix, oracle.align_reads_batch(ho, pool, *p, threads=8), batch, idx, p[-1], ("second pass raw", rl),
              lambda b: ix.align_reads_batch(b, *p))


# ---- b. chunk rollover with retired tails --------------------------------------------------------------------------------------
def rollover_pool(oracle, ho, chroms, k, min_core_len, max_num_slides):
    """4096 reads of 100 bp without N: one in ten exact, the others with 1..6 substitutions.  So that the batch stays in the step
    kernels they come from loci that align nowhere else and none of their probes can meet an N or an entry's end."""
    cand, truth = synth.make_reads(chroms[:3], 16000, 100, seed=4001, fixed_subs=5)
    eo = oracle.kalign_batch(ho, cand, threads=8, max_subs=5, max_ml=10, pe_mode=1)["out"]
    # the last phase (up to 5 mismatches) met this locus only, and nothing else within 6: NxtLowMMCnt is still its start value
    alone = (eo["hit_rslt"] == 1) & (eo["inst"] == 1) & (eo["low_mm"] == 5) & (eo["nxt_mm"] == 7)
    rng = np.random.default_rng(4002)
    reads = []
    for i, (c, start, strand, _) in enumerate(truth[alone]):
        r = chroms[c - 1][start:start + 100].copy()
        if r.max() > 3:
            continue
        subs = 0 if i % 10 == 0 else 1 + (i % 6)
        pos = rng.choice(100, size=subs, replace=False)
        r[pos] = (r[pos] + rng.integers(1, 4, size=subs)) % 4
        reads.append(synth.revcomp(r) if strand else r)
    clean = bb.never_probes_an_exception(reads, chroms, k, bb.kalign_core_offsets(100, 5, min_core_len, max_num_slides))
    pool = [reads[i] for i in np.nonzero(clean)[0][:4096]]
    assert len(pool) == 4096
    return pool


def check_rollover_batch(ix, oracle, ho, pool, batch, idx, kw):
    n, m = len(idx), len(idx) // len(pool)
    assert n == N_ROLLOVER == m * len(pool) and n > 8 * G and bb.fits(n, 4, False)
    po = oracle.kalign_batch(ho, pool, threads=8, **kw)
    o = po["out"]
    survive = ~(np.isin(o["hit_rslt"], (1, 2, 3)) & (o["low_mm"] == 0))  # not finalised by the exact phase
    share = survive.mean()
    assert 0.85 <= share <= 0.95, share
    per_pass = 64 * share
    model = bb.slot_model(n, 4, int(per_pass))
    assert 54 <= per_pass <= 61 and model["out_slots"] == 2 * 8192 * 512  # every wave rolls over: its first chunk ends in a retired tail
    assert sorted(set(np.where(o["hit_rslt"] == 1, o["low_mm"], 6).tolist())) == [0, 1, 2, 3, 4, 5, 6]  # the later steps get their shares
    ix.reset_counters()
    run_tiled(ix, po, batch, idx, kw["max_ml"], ("rollover", kw), lambda b: ix.kalign_batch(b, **kw))
    c = ix.counters()
    assert c["n_reads"] == n and c["n_bases"] == 100 * n, c
    assert c["n_lookup"] == m * po["counters"]["n_lookup"] and c["n_cand"] == m * po["counters"]["n_cand"], (c, po["counters"])
    assert c["n_slow"] < n // 100, c


@pytest.fixture(scope="module")
def rollover(oracle, g1):
    ix, ho, chroms = g1
    assert ix.min_core_len(0) == oracle.min_core_len(ho, 0)
    pool = rollover_pool(oracle, ho, chroms, ix.info()["kmer_k"], *ix.min_core_len(0))
    batch, idx = batch_of(pool, N_ROLLOVER, seed=95)
    return pool, batch, idx


def test_chunk_rollover_with_retired_tails(k4, oracle, g1, rollover):
    ix, ho, _ = g1
    check_rollover_batch(ix, oracle, ho, *rollover, KALIGN[0])


# ---- e. batches of shrinking size on one handle (and b's second parameter set) -------------------------------------------------
def test_shorter_batches_after_a_long_one(k4, oracle, golden_dir, g1, rollover):
    """stale ids and rows behind a shorter list are never read and ctl is reset: 5 M reads, then G + 4097, then 70, on a handle of
    their own, each exact"""
    _, ho, chroms = g1
    ix = k4.SfxIndex.open(os.path.join(golden_dir, "g1.sfx"))
    try:
        ix.set_max_iter(5000)
        kw = KALIGN[1]
        check_rollover_batch(ix, oracle, ho, *rollover, kw)
        pool = class_pool(chroms, 100)
        po = oracle.kalign_batch(ho, pool, threads=8, **kw)
        for n in (N_SECOND_PASS, 70):
            batch, idx = bb.tile(pool, n // len(pool), seed=n, tail=n % len(pool)) if n > len(pool) else bb.tile(pool[:n], 1, seed=n)
            run_tiled(ix, po, batch, idx, kw["max_ml"], ("after a long batch", n), lambda b: ix.kalign_batch(b, **kw))
    finally:
        ix.close()


# ---- c. deferred launch at scale -----------------------------------------------------------------------------------------------
FAMILY = dict(copies=1040, copy_len=150, slot=250, div=0.25)


def family_genome():
    """one 260 kbp entry (k-mer table of 9-mers) with 1040 copies of a 150 bp family, every base of a copy substituted with
    probability 0.25, either orientation: 9-mers of the family's consensus fill buckets far deeper than K4_DEEP_BUCKET, while a
    core of 20 bases or more of one copy is found in few others -- the reads stay in the step kernels.  Returns the copy starts too."""
    f = FAMILY
    names, chroms = synth.make_genome([f["copies"] * f["slot"]], seed=7301)
    rng = np.random.default_rng(7302)
    fam = rng.integers(0, 4, size=f["copy_len"], dtype=np.uint8)
    starts = np.arange(f["copies"]) * f["slot"]
    for p in starts:
        copy = fam.copy()
        m = rng.random(f["copy_len"]) < f["div"]
        copy[m] = (copy[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
        chroms[0][p:p + f["copy_len"]] = synth.revcomp(copy) if rng.random() < 0.5 else copy
    return names, chroms, starts


def family_pool(chroms, starts, counts, k):
    """4096 reads of 100 bp: nine in ten from inside the copies, with 1..4 substitutions behind the first k bases, chosen so that
    the read begins with a k-mer of a deep bucket; one in ten from the sequence between the copies"""
    f = FAMILY
    rng = np.random.default_rng(7303)
    g = chroms[0]
    pool = []
    while len(pool) < 3686:
        p = int(starts[rng.integers(0, len(starts))]) + int(rng.integers(0, f["copy_len"] - 100 + 1))
        r = g[p:p + 100].copy()
        if rng.random() < 0.5:
            r = synth.revcomp(r)
        if counts[bb.kmer_code(r, k)] <= bb.K4_DEEP_BUCKET:
            continue
        subs = 1 + len(pool) % 4
        pos = k + rng.choice(100 - k, size=subs, replace=False)
        r[pos] = (r[pos] + rng.integers(1, 4, size=subs)) % 4
        pool.append(r)
    while len(pool) < 4096:
        p = int(starts[rng.integers(0, len(starts))]) + f["copy_len"] + int(rng.integers(0, f["slot"] - f["copy_len"] - 100 + 1))
        r = g[p:p + 100].copy()
        subs = len(pool) % 3
        pos = rng.choice(100, size=subs, replace=False)
        r[pos] = (r[pos] + rng.integers(1, 4, size=subs)) % 4
        pool.append(synth.revcomp(r) if rng.random() < 0.5 else r)
    return pool


@pytest.fixture(scope="module")
def family(k4, oracle):
    names, chroms, starts = family_genome()
    ix, ho = index_from_oracle(k4, oracle, names, chroms)
    k = ix.info()["kmer_k"]
    counts = bb.kmer_counts(chroms, k)
    pool = family_pool(chroms, starts, counts, k)
    yield ix, ho, chroms, counts, k, pool
    ix.close()
    oracle.close(ho)


@pytest.mark.parametrize("kw", KALIGN, ids=["ml1", "ml10pe"])
@pytest.mark.parametrize("n", [N_SECOND_PASS, N_ROLLOVER])
def test_deferred_launch_at_scale(k4, oracle, family, n, kw):
    ix, ho, chroms, counts, k, pool = family
    # the first launch is split: the share of k-mer occurrences in deep buckets is ten times K4_DEFER_MIN_FRAC or more
    deep = counts > bb.K4_DEEP_BUCKET
    assert counts[deep].sum() / counts.sum() >= 0.02 >= 10 * bb.K4_DEFER_MIN_FRAC
    # and most reads are set aside by it: the '+' pass of phase one looks up the read's first k bases
    set_aside = np.array([counts[bb.kmer_code(r, k)] > bb.K4_DEEP_BUCKET for r in pool])
    assert set_aside.mean() >= 0.85 and len(pool) == 4096 and all(len(r) == 100 and r.max() <= 3 for r in pool)
    assert n > G and bb.fits(n, 4, True)
    model = bb.slot_model(n, 4, 64, int(64 * set_aside.mean()))
    assert model["passes"] >= 2 and model["defer_slots"] == (2 if n > 8 * G else 1) * 8192 * 512  # n > 8 G: the deferred list rolls over
    po = oracle.kalign_batch(ho, pool, threads=8, **kw)
    assert (po["out"]["nar"] == 1).mean() > 0.5
    batch, idx = batch_of(pool, n, seed=n % 1000)
    ix.reset_counters()
    run_tiled(ix, po, batch, idx, kw["max_ml"], ("deferred", n, kw), lambda b: ix.kalign_batch(b, **kw))
    c = ix.counters()
    assert c["n_reads"] == n and c["n_bases"] == 100 * n, c
    assert c["n_slow"] < n // 5, c  # most of the batch stays in the step kernels


# ---- d. general-kernel queues longer than their waves --------------------------------------------------------------------------
def test_slow_list_longer_than_its_waves(k4, oracle, g1):
    ix, ho, chroms = g1
    n = 40960
    pool = synth.make_reads(chroms[:3], 2780, 100, seed=8101, sub_lambda=1.5, edge_frac=0.03)[0]
    rng = np.random.default_rng(8102)
    for r in synth.make_reads(chroms[:3], 1230, 100, seed=8103, sub_lambda=1.5)[0]:  # 30 % of the pool: one N -> the general kernel
        r[int(rng.integers(0, 100))] = 4
        pool.append(r)
    for rl in (600, 900):  # too long for the step kernels
        pool += synth.make_reads(chroms[:3], 43, rl, seed=rl, sub_lambda=4.0)[0]
    assert len(pool) == 4096 and bb.fits(n, 16, False)
    batch, idx = bb.tile(pool, n // 4096, seed=81)
    n_general = (np.array([len(r) > 512 or (r == 4).any() for r in pool])[idx]).sum()
    assert n_general > bb.K4_SLOW_WAVES + 3000
    kw = dict(max_subs=5, max_ml=10, pe_mode=1)
    p = RAW_SETS[0]
    for what, po, mh, call in (("kalign", oracle.kalign_batch(ho, pool, threads=8, **kw), 10, lambda b: ix.kalign_batch(b, **kw)),
                               ("raw", oracle.align_reads_batch(ho, pool, *p, threads=8), p[-1], lambda b: ix.align_reads_batch(b, *p))):
        ix.reset_counters()
        run_tiled(ix, po, batch, idx, mh, ("slow list", what), call)
        assert ix.counters()["n_slow"] >= n_general > bb.K4_SLOW_WAVES, ix.counters()


def test_huge_list_longer_than_its_waves(k4, oracle):
    """the tandem-array genome of test_deep_repeats_vs_oracle: reads with more than 2047 candidates per strand pass outgrow the
    small dedupe tables and queue for the K4_HUGE_WAVES waves with the large ones"""
    rng = np.random.default_rng(77)
    c1 = rng.integers(0, 4, size=120000, dtype=np.uint8)
    c1[20000:27000] = np.resize(np.array([0, 2], np.uint8), 7000)           # (AG)n, 7 kb
    c1[60000:66000] = np.resize(np.array([1, 1, 3, 0, 2], np.uint8), 6000)  # 5-mer array, 6 kb
    c1[90000:94000] = 0                                                      # poly-A, 4 kb
    c2 = rng.integers(0, 4, size=50000, dtype=np.uint8)
    c2[10000:13000] = np.resize(np.array([0, 2], np.uint8), 3000)
    ix, ho = index_from_oracle(k4, oracle, ["chr1", "chr2"], [c1, c2])
    try:
        pool = []
        for j, start in enumerate(list(range(20100, 26800, 279)) + list(range(90100, 93800, 154)) + list(range(60100, 65800, 380))):
            r = c1[start:start + 100].copy()
            r[50] = (r[50] + 1) % 4  # one mismatch: no exact hit ends the walk early, every instance is counted
            pool.append(r if j % 2 else synth.revcomp(r))
        pool = pool[:64]
        assert len(pool) == 64
        n = 1024
        assert bb.fits(n, 4, True)
        batch, idx = bb.tile(pool, n // 64, seed=64)
        for (tm, cl, cd, sl, mh) in [(2, 33, 33, 8, 1), (3, 25, 25, 8, 10)]:
            po = oracle.align_reads_batch(ho, pool, tm, cl, cd, sl, 0, 1, 0, mh, threads=8)
            assert (po["inst"][idx] > 2047).sum() >= 300 > bb.K4_HUGE_WAVES, (po["inst"] > 2047).sum()
            run_tiled(ix, po, batch, idx, mh, ("huge list", tm, cl, mh), lambda b: ix.align_reads_batch(b, tm, cl, cd, sl, 0, 1, 0, mh))
    finally:
        ix.close()
        oracle.close(ho)
