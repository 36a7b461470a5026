"""The Python restatement of IterateExacts, MatchesOtherChroms and LocateSpeciesUniqueKMers (tests/kmarkers_ref.py) against what the
reference returned (tests/golden/kmarkers_calls.xz), field for field; kit4b_amd.kmarkers_fasta, fed from the restatement, against
the files the reference's front end wrote (tests/golden/kmarkers_<case>.fa.xz), byte for byte; each crafted site has the status it
was made for; the new symbols are declared.  No device."""
import io
import lzma
import os
import re

import numpy as np
import pytest

import kmarkers_craft as kc
import kmarkers_ref as kr
import query_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def load_calls(golden_dir):
    if "g" not in _cache:
        with lzma.open(os.path.join(golden_dir, "kmarkers_calls.xz"), "rb") as f:
            _cache["g"] = dict(np.load(io.BytesIO(f.read())))
    return _cache["g"]


def load_index(oracle, golden_dir, tmp_path_factory):
    """(path of the unpacked .sfx, (seq, sa, entries)), once per session"""
    if "ix" not in _cache:
        p = tmp_path_factory.mktemp("kmarkers") / "kmarkers_index.sfx"
        with lzma.open(os.path.join(golden_dir, "kmarkers_index.sfx.xz"), "rb") as f:
            p.write_bytes(f.read())
        h = oracle.open(str(p))
        _cache["ix"] = (str(p), query_ref.index_from_oracle(oracle, h))
        oracle.close(h)
    return _cache["ix"]


def probe_list(g):
    """[(codes, ids, MaxTotMM)] of the recorded probes"""
    return [(g["cat"][int(o):int(o) + int(l)], g["ids_cat"][int(a):int(b)].tolist(), int(m))
            for o, l, a, b, m in zip(g["offs"], g["lens"], g["ids_offs"][:-1], g["ids_offs"][1:], g["mm"])]


def scan_results(index):
    """{case name: (status bytes, tallies, markers)} of the restatement, computed once and shared with test_gpu_kmarkers.py"""
    if "scan" not in _cache:
        t = kc.target_ids()
        _cache["scan"] = {name: kr.species_kmers(index, t, **kw) for name, kw in kc.scan_cases()}
    return _cache["scan"]


@pytest.fixture(scope="module")
def index(oracle, golden_dir, tmp_path_factory):
    return load_index(oracle, golden_dir, tmp_path_factory)[1]


def test_the_index_is_the_crafted_one(index):
    names, seqs, _ = kc.build()
    seq, sa, entries = index
    assert len(entries) == 6 and [e[2] for e in entries] == [len(t) for t in seqs] and len(sa) == len(seq)
    for (eid, start, ln), t in zip(entries, seqs):
        assert bytes(b & 0x0F for b in seq[start:start + ln]) == t.tobytes()
    assert kc.target_ids() == [4, 2] and sorted(kc.TARGET_NAMES) != sorted(kc.TARGET_NAMES, key=str.lower)


def test_restatement_equals_the_recorded_returns(index, golden_dir):
    g = load_calls(golden_dir)
    pr = probe_list(g)
    assert len(pr) >= 300 and [p[0].tolist() for p in pr] == [p[0].tolist() for p in kc.probes(kc.build()[1])]
    n_hits = 0
    for i, (s, ids, mm) in enumerate(pr):
        a, b = int(g["walk_offs"][i]), int(g["walk_offs"][i + 1])
        want = list(zip(g["walk_idx"][a:b].tolist(), g["walk_entry"][a:b].tolist(), g["walk_loci"][a:b].tolist()))
        assert kr.walk_exacts(index, s.tobytes()) == want, i
        assert [w[0] for w in want] == list(range(want[0][0], want[0][0] + len(want))) if want else True  # one run of the array
        assert kr.matches_other_chroms(index, [ids[0]], mm, s.tobytes()) == int(g["m1"][i]), i
        assert kr.matches_other_chroms(index, ids, mm, s.tobytes()) == int(g["mn"][i]), i
        n_hits += len(want)
    assert n_hits > 300 and 0 < int(g["mn"].sum()) < len(pr) and max(b - a for a, b in zip(g["walk_offs"][:-1], g["walk_offs"][1:])) > 64
    # IterateExacts behind the last hit, and with a PrevHitIdx at the end of the array
    s = pr[0][0].tobytes()
    last = kr.walk_exacts(index, s)[-1][0]
    assert kr.iterate_exacts(index, s, last) == (0, 0, 0) and kr.iterate_exacts(index, s, len(index[1])) == (0, 0, 0)


@pytest.mark.parametrize("stem,kw", kc.file_cases())
def test_kmarkers_fasta_equals_the_front_end(index, golden_dir, stem, kw):
    import kit4b_amd

    with lzma.open(os.path.join(golden_dir, stem + ".fa.xz"), "rb") as f:
        want = f.read()
    got = kit4b_amd.kmarkers_fasta(kr.RefIndex(index, kc.NAMES), kc.CULTIVAR, kc.TARGET_NAMES, **kw)
    assert got == want, (stem, got[:200], want[:200])


def test_the_recorded_files_are_not_vacuous(golden_dir):
    sizes = {}
    for stem, kw in kc.file_cases():
        with lzma.open(os.path.join(golden_dir, stem + ".fa.xz"), "rb") as f:
            sizes[stem] = f.read().count(b">")
    assert sizes["kmarkers_k20_m0"] > 1000 and 2 <= sizes["kmarkers_k20_m1"] < 50 and sizes["kmarkers_k50_m2_p20_s2_K1"] > 5
    assert sizes["kmarkers_k50_m2_p20_s0_K3"] == 1 and sizes["kmarkers_k50_m2_p20_s3_K3"] == 0  # -K is the shared-prefix count, -s the Hamming


def test_each_crafted_site_has_its_status(index):
    res = scan_results(index)
    names, seqs, sites = kc.build()
    t = kc.target_ids()
    base = {t[0]: 0, t[1]: len(seqs[t[0] - 1])}

    def st(case, site, ofs=0):
        eid, loc = sites[site]
        return res[case][0][base[eid] + loc + ofs]

    for k in (20, 25, 50):
        c = "k%d_h1_m0" % k
        assert st(c, "acc") == kr.ACCEPTED
        assert st(c, "dup") == kr.ACCEPTED and st(c, "dup_again") == kr.DUPLICATE and st(c, "dup_b") == kr.DUPLICATE
        assert st(c, "rcdup") == kr.ACCEPTED and st(c, "rcdup_b") == kr.DUPLICATE  # (its first K bases are the complement of the site's last K)
        if k % 2 == 0:
            assert st(c, "pal_n", 1 + (50 - k) // 2) == kr.DUPLICATE  # the centred window: its own reverse complement, never reported
        assert st(c, "rcf1") == kr.ACCEPTED   # the only antisense hit is the first, which the walk skips
        assert st(c, "rcf2") == kr.FOREIGN_HIT
        assert st(c, "ff") == kr.FIRST_FOREIGN and st(c, "fh") == kr.FOREIGN_HIT
        homo = [st(c, "homo_c", 1 + i) for i in range(151 - k)]  # C, 150 A, G: a run of 151 - k elements
        assert homo == [kr.ACCEPTED] + [kr.DUPLICATE] * (150 - k) and 151 - k > 64
        n0 = "nruns_%d" % k  # N, K - 1 bases, N, K bases, N, K + 1 bases, N
        assert [st(c, n0, i) for i in range(3 * k + 4)] == [1] * (k + 1) + [7] + [1] * k + [7, 7] + [1] * k
        assert res[c][0][-1] == kr.NOT_KMER
    # the entries' ends: tgt_A ends with N + 20 bases, Tgt_b with N + 51
    la, lb = len(seqs[3]), len(seqs[1])
    assert list(res["k20_h1_m0"][0][la - 21:la]) == [1, 7] + [1] * 19 and list(res["k25_h1_m0"][0][la - 21:la]) == [1] * 21
    assert list(res["k50_h1_m0"][0][la + lb - 52:]) == [1, 7, 7] + [1] * 49
    # Hamming, K = 50: MinHamming 3 has cores of 16 at 0, 16 and 32; MinHamming 2 one core of 25 at 0
    h3, h2 = "k50_h3_m0", "k50_h2_m0"
    assert st(h3, "ham1") == kr.HAMMING and st(h2, "ham1") == kr.ACCEPTED
    assert st(h3, "ham_start") == kr.ACCEPTED and st(h3, "ham_end") == kr.ACCEPTED  # the probe cannot be laid over the hit inside the entry
    assert st(h2, "ham_last") == kr.ACCEPTED and st(h3, "ham_last") == kr.HAMMING   # bases 25..49: the core MinHamming 2 never looks at
    assert st(h3, "ham_rc") == kr.HAMMING and st(h2, "ham_rc") == kr.ACCEPTED
    assert st(h2, "rcf1") == kr.HAMMING  # (what the skipped antisense hit lets through, the core walk finds)
    assert kr.HAMMING in res["k20_h5_m0"][0] and res["k20_h5_m0"][1][2] < res["k20_h2_m0"][1][2] < res["k20_h1_m0"][1][2] == res["k20_h1_m0"][1][1]
    # prefixes, K = 50, 20 bases: shared with 0, 1 and 3 other entries, the third only as the reverse complement
    for s, want in ((1, (6, 7, 7)), (3, (6, 6, 7)), (0, (6, 6, 6))):
        c = "k50_h1_m2_s%d" % s
        assert (st(c, "acc"), st(c, "px1"), st(c, "px3")) == want, c
    assert st("k50_h2_m2_s3", "px3") == kr.ACCEPTED
    # mode 1, K = 20: accepted runs of 1, 2 and 5 with duplicates between; each is written because an accepted K-mer follows
    got = [res["k20_h1_m1"][0][base[2] + sites["runs"][1] + i] for i in range(len(kc.RUN_PATTERN))]
    assert got == [kr.ACCEPTED if c == "A" else kr.DUPLICATE for c in kc.RUN_PATTERN]
    stretch = seqs[1][sites["runs"][1]:sites["runs"][1] + len(kc.RUN_PATTERN) + 19].tobytes()
    markers = res["k20_h1_m1"][2]
    for i, ln in ((1, 1), (3, 2), (6, 5)):
        assert stretch[i:i + 19 + ln] in markers
    assert res["k20_h1_m1"][1][3] == len(markers) < res["k20_h1_m0"][1][3] == int((np.frombuffer(res["k20_h1_m0"][0], np.uint8) == 7).sum())
    for name, (status, tallies, _) in res.items():
        a = np.frombuffer(status, np.uint8)
        assert tallies[:3] == [int((a > 1).sum()), int((a > 4).sum()), int((a > 5).sum())] and a.min() >= 1 and a.max() <= 7, name
    assert res["k100_h5_m0"][1][0] > 0


def test_parameter_errors_of_the_restatement(index):
    for name, t, kw in kc.error_cases():
        kw = dict(dict(min_hamming=1, mode=0, prefix_len=0), **kw)
        assert kr.check_params(index, t or kc.target_ids(), kw["kmer_len"], kw["min_hamming"], kw["mode"], kw["prefix_len"]) == kr.ERR_PARAMS, name
    assert kr.check_params(index, kc.target_ids(), 20, 1, 2, 10) == 0


def test_new_symbols_are_declared_and_bound():
    import kit4b_amd

    header = open(os.path.join(ROOT, "include", "k4sfx.h")).read()
    names = ["k4_exact_ranges_batch", "k4_exact_ranges_batch_dev", "k4_matches_other_chroms_batch", "k4_species_kmers_batch",
             "k4_species_kmers_batch_dev", "k4_kmarkers_last_kernel_ms"]
    src = open(os.path.join(ROOT, "kit4b_amd", "csrc", "k4_kmarkers.hip")).read()
    for n in names:
        assert re.search(r"\b%s\(" % n, header) and re.search(r'extern "C" \w+ %s\(' % n, src), n
    assert "k4_kmarkers.hip" in open(os.path.join(ROOT, "kit4b_amd", "csrc", "Makefile")).read()
    for n in ("kmarkers_fasta", "KMarkersParams", "KMarkersTotals"):
        assert hasattr(kit4b_amd, n), n
    for n in ("exact_ranges", "matches_other_chroms", "species_kmers"):
        assert hasattr(kit4b_amd.SfxIndex, n), n
    facade = open(os.path.join(ROOT, "include", "k4_sfxarray.hpp")).read()
    for n in ("IterateExacts", "MatchesOtherChroms", "SpeciesKMersBatch"):
        assert n in facade, n
