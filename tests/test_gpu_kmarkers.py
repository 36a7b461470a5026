"""kmarkers on the device (k4_kmarkers.hip) through the C ABI, the Python binding and the C++ facade: exact ranges and
MatchesOtherChroms against the reference's recorded returns, the species scan against the Python restatement that
test_kmarkers_cpu.py pins to those recordings, and kmarkers_fasta against the front end's recorded files."""
import ctypes as C
import lzma
import os
import subprocess

import numpy as np
import pytest

import cults_craft as cc
import kmarkers_craft as kc
import kmarkers_ref as kr
import runlen_craft as rc
from test_cults_cpu import big_index
from test_kmarkers_cpu import load_calls, load_index, probe_list, scan_results

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALLIES = ("processed", "cultivar_specific", "hamming_retained", "accepted")


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


@pytest.fixture(scope="module")
def crafted(oracle, golden_dir, tmp_path_factory):
    return load_index(oracle, golden_dir, tmp_path_factory)


@pytest.fixture(scope="module")
def ix(k4, crafted):
    x = k4.SfxIndex.open(crafted[0])
    yield x
    x.close()


def test_exact_ranges_equal_the_recorded_walks(ix, golden_dir):
    g = load_calls(golden_dir)
    pr = probe_list(g)
    firsts, counts = ix.exact_ranges([p[0] for p in pr])
    assert ix.kmarkers_kernel_ms() > 0
    for i in range(len(pr)):
        a, b = int(g["walk_offs"][i]), int(g["walk_offs"][i + 1])
        assert int(counts[i]) == b - a, i
        assert int(firsts[i]) == (int(g["walk_idx"][a]) - 1 if b > a else 0), i
    assert int(counts.max()) > 64 and int((counts == 0).sum()) > 20
    f0, c0 = ix.exact_ranges([])
    assert len(f0) == 0 and ix.kmarkers_kernel_ms() == 0


def test_exact_ranges_dev_form_and_untouched_bytes(k4, ix, golden_dir):
    g = load_calls(golden_dir)
    L = k4.lib()
    n = len(g["lens"])
    want_f, want_c = ix.exact_ranges((g["cat"], g["offs"], g["lens"]))
    arrays = [np.concatenate([g["cat"], np.zeros(16, np.uint8)]), g["offs"].astype(np.uint64), g["lens"].astype(np.uint32),
              np.full(8 * (n + 2), 0xEE, np.uint8), np.full(4 * (n + 2), 0xEE, np.uint8)]
    d = [C.c_void_p() for _ in arrays]
    try:
        for ptr, a in zip(d, arrays):
            assert L.k4_alloc_device(ix.h, a.nbytes, C.byref(ptr)) == 0
            assert L.k4_copy_to_device(ix.h, ptr, a.ctypes.data, a.nbytes) == 0
        assert L.k4_exact_ranges_batch_dev(ix.h, n, d[0], d[1], d[2], d[3], d[4], None) == 0
        for ptr, a in zip(d[3:], arrays[3:]):
            assert L.k4_copy_to_host(ix.h, a.ctypes.data, ptr, a.nbytes) == 0
    finally:
        for ptr in d:
            L.k4_free_device(ptr)
    assert np.array_equal(arrays[3][:8 * n].view(np.uint64), want_f) and np.array_equal(arrays[4][:4 * n].view(np.uint32), want_c)
    assert (arrays[3][8 * n:] == 0xEE).all() and (arrays[4][4 * n:] == 0xEE).all()


def test_matches_other_chroms_equal_the_recorded_returns(ix, golden_dir):
    g = load_calls(golden_dir)
    pr = probe_list(g)
    groups = {}
    for i, (s, ids, mm) in enumerate(pr):
        groups.setdefault((tuple(ids), mm), []).append(i)
        groups.setdefault(((ids[0],), mm), [])
    got_n, got_1 = np.zeros(len(pr), np.int32), np.zeros(len(pr), np.int32)
    for (ids, mm), members in groups.items():
        if members:
            got_n[members] = ix.matches_other_chroms(list(ids), mm, [pr[i][0] for i in members])
    for i, (s, ids, mm) in enumerate(pr):  # the single-id overload, each a batch of one for a third of the probes
        got_1[i] = ix.matches_other_chroms(ids[0], mm, [s])[0] if i % 3 == 0 else g["m1"][i]
    assert np.array_equal(got_n, g["mn"]) and np.array_equal(got_1, g["m1"]) and 0 < int(g["mn"].sum()) < len(pr)


def test_species_kmers_equal_the_restatement(ix, crafted):
    res = scan_results(crafted[1])
    t = kc.target_ids()
    for name, kw in kc.scan_cases():
        status, tallies = ix.species_kmers(t, **kw)
        want = np.frombuffer(res[name][0], dtype=np.uint8)
        assert status.shape == want.shape and np.array_equal(status, want), (name, np.flatnonzero(status != want)[:5])
        assert [tallies[k] for k in TALLIES] == res[name][1], name
        assert ix.kmarkers_kernel_ms() > 0


def test_species_kmers_parameter_errors(k4, ix):
    for name, t, kw in kc.error_cases():
        with pytest.raises(k4.K4Error) as e:
            ix.species_kmers(t or kc.target_ids(), **kw)
        assert e.value.code == kr.ERR_PARAMS, name
        assert ix.kmarkers_kernel_ms() == 0


@pytest.mark.parametrize("stem,kw", kc.file_cases())
def test_kmarkers_fasta_equals_the_front_end(k4, ix, golden_dir, stem, kw):
    with lzma.open(os.path.join(golden_dir, stem + ".fa.xz"), "rb") as f:
        want = f.read()
    assert k4.kmarkers_fasta(ix, kc.CULTIVAR, kc.TARGET_NAMES, **kw) == want, stem


def test_species_kmers_dev_form_and_untouched_bytes(k4, ix, crafted):
    res = scan_results(crafted[1])
    L = k4.lib()
    t = np.array(kc.target_ids(), dtype=np.uint32)
    for name in ("k20_h2_m1", "k50_h2_m2_s3"):
        kw = dict(kc.scan_cases())[name]
        want = np.frombuffer(res[name][0], dtype=np.uint8)
        n = len(want)
        p = k4.KMarkersParams(kw["kmer_len"], kw["min_hamming"], kw["mode"], kw.get("prefix_len", 0), kw.get("min_with_prefix", 0), 0)
        host = np.full(n + 64, 0xEE, dtype=np.uint8)
        tot = k4.KMarkersTotals()
        assert L.k4_species_kmers_batch(ix.h, C.byref(p), 2, t.ctypes.data, host.ctypes.data, n + 64, C.byref(tot)) == 0
        assert np.array_equal(host[:n], want) and (host[n:] == 0xEE).all()
        assert L.k4_species_kmers_batch(ix.h, C.byref(p), 2, t.ctypes.data, host.ctypes.data, n - 1, C.byref(tot)) == kr.ERR_PARAMS
        dev = np.full(n + 64, 0xEE, dtype=np.uint8)
        d, tot2 = C.c_void_p(), k4.KMarkersTotals()
        assert L.k4_alloc_device(ix.h, n + 64, C.byref(d)) == 0
        try:
            assert L.k4_copy_to_device(ix.h, d, dev.ctypes.data, n + 64) == 0
            assert L.k4_species_kmers_batch_dev(ix.h, C.byref(p), 2, t.ctypes.data, d, n + 64, C.byref(tot2), None) == 0
            assert L.k4_copy_to_host(ix.h, dev.ctypes.data, d, n + 64) == 0
        finally:
            L.k4_free_device(d)
        assert np.array_equal(dev, host)
        assert [getattr(tot2, k) for k in TALLIES] == [getattr(tot, k) for k in TALLIES] == res[name][1]


def test_a_second_index_on_the_same_file_gives_the_same_statuses(k4, ix, crafted):
    """nothing was written into the index: an index opened after the first has run its scans answers alike"""
    res = scan_results(crafted[1])
    first, _ = ix.species_kmers(kc.target_ids(), 20, 2, 0)
    y = k4.SfxIndex.open(crafted[0])
    try:
        second, _ = y.species_kmers(kc.target_ids(), 20, 2, 0)
        for e in (2, 4):
            n = ix.entry(e)["seq_len"]
            assert np.array_equal(ix.get_seq(e, 0, n), y.get_seq(e, 0, n)) and int(ix.get_seq(e, 0, n).max()) <= 4  # no flag bits
    finally:
        y.close()
    again, _ = ix.species_kmers(kc.target_ids(), 20, 2, 0)
    want = np.frombuffer(res["k20_h2_m0"][0], dtype=np.uint8)
    assert np.array_equal(first, want) and np.array_equal(second, want) and np.array_equal(again, want)


def test_big_targets_past_one_launch(k4, oracle, tmp_path_factory):
    """cults_craft.big_targets(): 6 x 17 000 bases, two targets, 34 000 start loci -- three launches of the scan (16 384 waves each),
    and cultivars 3 % apart, so most K-mers of a target meet the other cultivars' copies"""
    names, ts = cc.big_targets()
    h = oracle.build(names, ts, dataset="cultsbig", threads=4)
    p = tmp_path_factory.mktemp("kmbig") / "kmarkers_big.sfx"
    oracle.write(h, str(p))
    oracle.close(h)
    ref = big_index(oracle)
    want, tallies, _ = kr.species_kmers(ref, [5, 2], 20, 2, 1)
    x = k4.SfxIndex.open(str(p))
    try:
        status, tot = x.species_kmers([5, 2], 20, 2, 1)
    finally:
        x.close()
    assert np.array_equal(status, np.frombuffer(want, np.uint8)) and [tot[k] for k in TALLIES] == tallies
    assert len(status) == 34000 and tallies[3] > 20 and tallies[1] > tallies[2] > 0


@pytest.mark.parametrize("r", rc.RUN_LENGTHS)
def test_runs_that_end_at_a_turn_of_the_walk(k4, oracle, r):
    """runlen_craft.kmarkers_runs(r): two 24-mers of exactly r occurrences, the one foreign occurrence at rank 0 of the run (the first
    lane of the first turn of 64 suffixes) or at rank r - 1 (the last lane of the last turn, which ends before, at or behind a full
    turn).  Exact ranges, MatchesOtherChroms and the species scan in mode 2 (prefix 12: the prefix pass walks the same runs from the
    K-mer that shares its prefix with them) against the restatements."""
    names, chroms, km = rc.kmarkers_runs(r)
    with rc.host_index(k4, oracle, names, chroms) as (x, ref):
        probes = [km["first"], km["last"], km["fork"], km["first"][:12], km["last"][:23]]
        firsts, counts = x.exact_ranges(probes)
        for p, f, c in zip(probes, firsts, counts):
            walk = kr.walk_exacts(ref, p.tobytes())
            assert int(c) == len(walk) and int(f) == (walk[0][0] - 1 if walk else 0), (r, int(f), int(c))
        assert counts[:4].tolist() == [r, r, 1, r + 1]
        # one core of 24 (probes of 48 bases, MaxTotMM 1) and cores of 8 (24 bases, MaxTotMM 2), in front of the target's occurrences
        t = chroms[0].tobytes()
        long_probes = [chroms[0][at:at + 48] for m in (km["first"], km["last"]) for at in (t.find(m.tobytes()), t.rfind(m.tobytes()))]
        for ids in ([1], [1, 2], [1, 3]):
            for mm, ps in ((1, long_probes), (2, probes[:3])):
                got = x.matches_other_chroms(ids, mm, ps)
                want = [kr.matches_other_chroms(ref, ids, mm, p.tobytes()) for p in ps]
                assert got.tolist() == want, (r, ids, mm)
        assert x.matches_other_chroms([1], 1, long_probes).tolist() == [1 if r > 1 else 0] * 4
        for mwp in (0, 1):
            want, tallies, _ = kr.species_kmers(ref, [1], 24, 1, 2, 12, mwp)
            status, tot = x.species_kmers([1], 24, 1, 2, 12, mwp)
            assert np.array_equal(status, np.frombuffer(want, np.uint8)) and [tot[k] for k in TALLIES] == tallies, (r, mwp)
        if r > 1:  # (with one foreign entry asked for: first's occurrences, last's first and later ones, fork)
            assert {kr.FIRST_FOREIGN, kr.FOREIGN_HIT, kr.DUPLICATE, kr.ACCEPTED} <= set(status.tolist())


def test_csfxarray_kmarkers_facade_program(crafted, golden_dir, tmp_path):
    """CSfxArray::IterateExacts walked to exhaustion, both MatchesOtherChroms overloads and SpeciesKMersBatch of include/k4_sfxarray.hpp"""
    exe = os.path.join(ROOT, "kit4b_amd", "k4_kmarkers_facade_test")
    assert os.path.exists(exe), "make -C kit4b_amd/csrc"
    g = load_calls(golden_dir)
    lines = []
    for i, (s, ids, mm) in enumerate(probe_list(g)[::3]):
        i *= 3
        a, b = int(g["walk_offs"][i]), int(g["walk_offs"][i + 1])
        hits = " ".join("%d %d %d" % (g["walk_idx"][k], g["walk_entry"][k], g["walk_loci"][k]) for k in range(a, b))
        lines.append("%d %s %d %s %d %d %d %d %s" % (len(s), "".join(str(int(c)) for c in s), len(ids), " ".join(map(str, ids)), mm, g["m1"][i], g["mn"][i], b - a, hits))
    (tmp_path / "calls.txt").write_text("\n".join(lines) + "\n")
    name = "k50_h2_m2_s3"
    kw = dict(kc.scan_cases())[name]
    status, tallies, _ = scan_results(crafted[1])[name]
    t = kc.target_ids()
    (tmp_path / "scan.txt").write_text("%d %d %d %d %d %d %s %d %d %d %d %d\n%s\n" % (
        kw["kmer_len"], kw["min_hamming"], kw["mode"], kw["prefix_len"], kw["min_with_prefix"], len(t), " ".join(map(str, t)), *tallies, len(status),
        "".join(str(c) for c in status)))
    out = subprocess.run([exe, crafted[0], str(tmp_path / "calls.txt"), str(tmp_path / "scan.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.splitlines()
    n_hits = sum(int(g["walk_offs"][i + 1] - g["walk_offs"][i]) for i in range(0, len(g["lens"]), 3))
    assert got == ["probes %d hits %d bad walks 0 bad single 0 bad list 0" % (len(lines), n_hits), "scan 0 bad 0 tallies 1 fill 1", "errors -100 -100 msgs 2"], got
