"""The step kernels' per-length plan table, the read packing and the coarse start of the entry lookup (-m gpu), read for
read against the CPU oracle: every read length of every length class in one batch, N / invalid symbols at the packing's word
and chunk boundaries, and reads at the edges of the entries of many-entry genomes."""
import ctypes as C
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


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


def same_kalign(eg, eo, max_ml, what):
    bad = np.nonzero(eo["out"] != eg["out"])[0]
    assert len(bad) == 0, (what, bad[:8], eg["out"][bad[:8]], eo["out"][bad[:8]])
    for i in range(len(eo["out"])):
        r = eo["out"][i]
        nh = min(int(r["inst"]), max_ml) if r["hit_rslt"] in (1, 2, 3) else 0
        assert np.array_equal(eo["hits"][i, :nh], eg["hits"][i, :nh]), (what, i)


def same_raw(rg, ro, max_hits, what):
    for k in ("rslt", "inst", "low", "nxt"):
        bad = np.nonzero(rg[k] != ro[k])[0]
        assert len(bad) == 0, (what, k, bad[:8], rg[k][bad[:8]], ro[k][bad[:8]])
    for i in range(len(ro["rslt"])):
        nh = min(int(ro["inst"][i]), max_hits) if ro["rslt"][i] in (1, 2, 3) else 0
        assert np.array_equal(rg["hits"][i, :nh], ro["hits"][i, :nh]), (what, i)
        assert not rg["hits"][i, nh:].view(np.uint8).any(), (what, i, "stale hit slots")


KALIGN_SETS = [dict(max_subs=s, min_edit_dist=d, max_ml=m, pe_mode=1 if m > 1 else 0)
               for s in (0, 2, 5, 10) for d in (1, 2) for m in (1, 10)]
# raw AlignReads sets (tot_mm, core_len, core_delta, max_slides, min_core_len, mm_delta, strand, max_hits): the first escalates
# through up to five phases, the second has two at most
RAW_SETS = [(4, 20, 20, 30, 0, 1, 0, 3), (1, 12, 12, 8, 0, 2, 0, 1)]


def every_length_reads(chroms):
    """three reads of each length 1..160 and of 161, 255, 256, 257, 511, 512, 513, back to back: the odd lengths move the
    start of the next read through every alignment modulo 4"""
    reads = []
    for rl in list(range(1, 161)) + [161, 255, 256, 257, 511, 512, 513]:
        r, _ = synth.make_reads(chroms[:3], 3, rl, seed=1000 + rl, sub_lambda=max(0.7, rl / 60.0) if rl >= 12 else 0.0,
                                n_prob=0.03 if rl >= 12 else 0.0, edge_frac=0.1)
        reads += r
    return reads


def check_batch(ix, oracle, ho, reads, what):
    for kw in KALIGN_SETS:
        eo = oracle.kalign_batch(ho, reads, threads=8, **kw)
        eg = ix.kalign_batch(reads, **kw)
        same_kalign(eg, eo, kw["max_ml"], (what, kw))
    for p in RAW_SETS:
        ro = oracle.align_reads_batch(ho, reads, *p, threads=8)
        rg = ix.align_reads_batch(reads, *p)
        same_raw(rg, ro, p[-1], (what, p))


@pytest.mark.parametrize("max_len", [513, 256, 160, 128])
def test_every_length_in_one_batch(k4, oracle, g1, max_len):
    """All lengths up to max_len in one batch: 513 runs the 16-word class (plan table in LDS) and sends 513 to the general
    kernel, 256 and 160 the 8- and 5-word classes (plan per lane), 128 the 4-word class (table)."""
    ix, ho, chroms = g1
    reads = [r for r in every_length_reads(chroms) if len(r) <= max_len]
    starts = np.cumsum([0] + [len(r) for r in reads[:-1]]) % 4
    assert set(starts.tolist()) == {0, 1, 2, 3}
    check_batch(ix, oracle, ho, reads, "lengths <= %d" % max_len)


def test_uniform_length_batch(k4, oracle, g1):
    """every read 100 bp: one plan record serves the whole batch"""
    ix, ho, chroms = g1
    reads, _ = synth.make_reads(chroms[:3], 1500, 100, seed=77, sub_lambda=2.0, n_prob=0.02, edge_frac=0.05, random_frac=0.03)
    check_batch(ix, oracle, ho, reads, "uniform 100")


def corner_reads(chroms):
    """reads from true loci of both strands carrying N (4) or an invalid symbol (5, 6, 7) at the packing's corners"""
    rng = np.random.default_rng(4711)
    reads = []
    for rl in (31, 32, 33, 64, 100, 127, 128):
        places = sorted({0, rl - 1} | {p for p in (31, 32, 63) if p < rl})
        edits = [[(p, 4)] for p in places]
        edits += [[(p, 5 + (j + k) % 3)] for j, p in enumerate(places) for k in range(2)]
        edits += [[(0, 4), (rl - 1, 4)], [(places[len(places) // 2], 4), (1, 4)], [(0, 4), (rl // 2, 4), (rl - 1, 4)],
                  [(2, 4), (3, 4), (rl - 2, 4)], [(0, 4), (rl - 1, 6)], []]
        for ed in edits:
            for strand in (0, 1):
                c = int(rng.integers(0, 3))
                start = int(rng.integers(0, len(chroms[c]) - rl + 1))
                rd = chroms[c][start:start + rl].copy()
                if strand:
                    rd = synth.revcomp(rd)
                for p, sym in ed:
                    rd[p] = sym
                reads.append(rd)
    return reads


@pytest.mark.parametrize("max_ns", [0, 1, 2])
def test_packing_corners(k4, oracle, g1, max_ns):
    """N and symbols above N at base 0, at the last base and at bases 31, 32 and 63 (the last base of a packed 64-bit word, the
    first of the next, the last of that one), one to three Ns around the MaxNs limit (1 is the default); AlignRead and raw"""
    ix, ho, chroms = g1
    reads = corner_reads(chroms)
    for kw in (dict(max_subs=5), dict(max_subs=10, max_ml=10, pe_mode=1, min_edit_dist=2)):
        eo = oracle.kalign_batch(ho, reads, threads=8, max_ns=max_ns, **kw)
        eg = ix.kalign_batch(reads, max_ns=max_ns, **kw)
        same_kalign(eg, eo, kw.get("max_ml", 1), ("corners", max_ns, kw))
    if max_ns == 1:  # AlignReads itself has no rule for N: the reads without a symbol above N (AlignRead lets no other through)
        reads = [r for r in reads if r.max() <= 4]
        for p in RAW_SETS:
            same_raw(ix.align_reads_batch(reads, *p), oracle.align_reads_batch(ho, reads, *p, threads=8), p[-1], ("corners raw", p))


def edge_reads(chroms, rl=50):
    """per entry: its first bases, its last possible bases, the read that would cross its end by one base, one inside"""
    rng = np.random.default_rng(99)
    reads = []
    for c in chroms:
        n = len(c)
        inside = int(rng.integers(0, n - rl + 1))
        cross = np.concatenate([c[n - rl + 1:], rng.integers(0, 4, size=1, dtype=np.uint8)])
        for rd in (c[:rl], c[n - rl:], cross, c[inside:inside + rl]):
            rd = rd.copy()
            if rng.random() < 0.3:
                p = int(rng.integers(20, rl - 1))
                rd[p] = (rd[p] + 1) % 4
            reads.append(synth.revcomp(rd) if rng.random() < 0.5 else rd)
    return reads


@pytest.mark.parametrize("n_entries", [60, 140])
def test_entry_lookup_at_entry_edges(k4, oracle, n_entries):
    """60 entries of 300 bp .. 200 kbp in shuffled order (several small entries inside one coarse block, a large one across
    many): the entry table is searched in LDS from the coarse start; 140 entries: the global table, as before"""
    rng = np.random.default_rng(n_entries)
    lens = np.geomspace(300, 200000 if n_entries == 60 else 40000, n_entries).astype(int)
    rng.shuffle(lens)
    names, chroms = synth.make_genome([int(x) for x in lens], seed=2024 + n_entries)
    ho = oracle.build(names, chroms, dataset="edges", threads=8)
    n = oracle.concat_len(ho)
    sa_raw = np.ctypeslib.as_array(C.cast(oracle.L.k4o_sa_bytes(ho), C.POINTER(C.c_uint8)), shape=(n * 4,))
    ix = k4.SfxIndex.from_host(np.array(oracle.seq(ho)), sa_raw, 4, k4.make_entries(names, [len(c) for c in chroms]), dataset="edges")
    try:
        assert ix.info()["n_entries"] == n_entries
        oracle.set_max_iter(ho, 5000)
        ix.set_max_iter(5000)
        reads = edge_reads(chroms)
        for kw in (dict(max_subs=2), dict(max_subs=5, max_ml=10, pe_mode=1)):
            eo = oracle.kalign_batch(ho, reads, threads=8, **kw)
            eg = ix.kalign_batch(reads, **kw)
            same_kalign(eg, eo, kw.get("max_ml", 1), ("edges", n_entries, kw))
        assert (eo["out"]["nar"] == 1).sum() > len(reads) // 2  # the in-entry reads are found
        p = RAW_SETS[0]
        same_raw(ix.align_reads_batch(reads, *p), oracle.align_reads_batch(ho, reads, *p, threads=8), p[-1], ("edges raw", n_entries))
    finally:
        ix.close()
        oracle.close(ho)
