"""K-mer cultivar counts on the device (k4_cults.hip) through the C ABI, the Python binding and the C++ facade, against the Python
restatement that test_cults_cpu.py pins to the reference's recorded callbacks: every crafted case with the default window and with
windows of 64 elements, the resumable protocol, indexes on both sides of the entry-lookup and histogram bounds, 5-byte elements."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cults_craft as cc
import cults_ref
import manytargets as mt
import query_ref
from test_cults_cpu import all_results, big_index, fasta_records, load_big, load_cases, load_index

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _same(k4, got, rc, recs, klen, what):
    want = cults_ref.as_arrays(k4, rc, recs, klen)
    assert got["n_located"] == want["n_located"], what
    for f in ("kmers", "bases", "dist"):
        assert got[f].shape == want[f].shape and np.array_equal(got[f], want[f]), (what, f, got[f][:3], want[f][:3])


def _call(x, kw, r, **more):
    return x.kmer_cults(kw["plen"], kw["slen"], kw["min_cult"], sense_only=kw["sense_only"], start_sfx_idx=r[0], end_sfx_idx=r[1],
                        max_homozygotic=kw["max_homo"], **more)


@pytest.mark.parametrize("window", [0, 64])
def test_every_crafted_case_equals_the_restatement(k4, ix, crafted, golden_dir, window):
    res = all_results(crafted[1], golden_dir)
    n_ok = 0
    for name, kw, _ in cc.cases():
        r, rc, recs = res[name]
        if r is None:
            continue
        if rc < 0:
            with pytest.raises(k4.K4Error) as e:
                _call(ix, kw, r, max_window=window)
            assert e.value.code == rc, name
            continue
        _same(k4, _call(ix, kw, r, max_window=window), rc, recs, kw["plen"] + kw["slen"], (name, window))
        assert (ix.cults_kernel_ms() > 0) == (r[0] < len(crafted[1][0])), name  # (a call without an element launches nothing)
        n_ok += 1
    assert n_ok == sum(1 for v in res.values() if v[0] is not None and v[1] >= 0) >= 20
    assert ix.cults_kernel_ms() == 0  # (the last case is a call the device turns down)


def test_resumable_with_room_for_one_kmer_and_untouched_bytes(k4, ix, crafted, golden_dir):
    """caps of one K-mer and of n_entries counts: the calls chained by next_sfx_idx write what one big call writes; the bytes
    behind the written records keep the caller's fill; the device-pointer form writes the same records"""
    res = all_results(crafted[1], golden_dir)
    L = k4.lib()
    for name, window in (("min3", 64), ("mid_run", 64), ("p5_s5", 0)):
        kw = [c for c in cc.cases() if c[0] == name][0][1]
        r, rc, recs = res[name]
        _same(k4, _call(ix, kw, r, max_window=window, max_kmers=1, max_dist=5), rc, recs, kw["plen"] + kw["slen"], name)
    name, kw, _ = cc.cases()[1]
    r, rc, recs = res[name]
    klen = kw["plen"] + kw["slen"]
    want = cults_ref.as_arrays(k4, rc, recs, klen)
    cap_k, cap_d = 7, 40
    p = k4.CultsParams(kw["plen"], kw["slen"], kw["min_cult"], 0, 64, 0)
    kmers = np.full(cap_k + 2, 0xEE, dtype=np.uint8).repeat(k4.CULT_KMER_DTYPE.itemsize)
    bases = np.full((cap_k + 2) * klen, 0xEE, dtype=np.uint8)
    dist = np.full((cap_d + 2) * 12, 0xEE, dtype=np.uint8)
    out = k4.CultsOut(kmers.ctypes.data, bases.ctypes.data, dist.ctypes.data)
    tot = k4.CultsTotals()
    assert L.k4_kmer_cults_batch(ix.h, C.byref(p), 0, 0, C.byref(out), C.byref(k4.CultsCaps(cap_k, cap_d)), C.byref(tot)) == 0
    nk, nd = tot.n_kmers, tot.n_dist
    assert 0 < nk <= cap_k and nd <= cap_d and not tot.done and (nk == cap_k or nd + 5 > cap_d)
    assert np.array_equal(kmers[:nk * 32].view(k4.CULT_KMER_DTYPE), want["kmers"][:nk])
    assert np.array_equal(bases[:nk * klen].reshape(nk, klen), want["bases"][:nk])
    assert np.array_equal(dist[:nd * 12].view(k4.CULT_DIST_DTYPE), want["dist"][:nd])
    assert (kmers[nk * 32:] == 0xEE).all() and (bases[nk * klen:] == 0xEE).all() and (dist[nd * 12:] == 0xEE).all()
    # next_sfx_idx is where the next reported K-mer's run starts or in front of it, and a run's start
    fl = cults_ref.flags(crafted[1], kw["plen"], kw["slen"], 0, int(tot.next_sfx_idx))
    assert fl[-1][2] and int(want["kmers"][nk - 1]["head_sfx_idx"]) < tot.next_sfx_idx <= int(want["kmers"][nk]["head_sfx_idx"])
    # the device-pointer form
    d = [C.c_void_p() for _ in range(3)]
    for ptr, a in zip(d, (kmers, bases, dist)):
        assert L.k4_alloc_device(ix.h, len(a), C.byref(ptr)) == 0
    tot2 = k4.CultsTotals()
    dout = k4.CultsOut(d[0].value, d[1].value, d[2].value)
    assert L.k4_kmer_cults_batch_dev(ix.h, C.byref(p), 0, 0, C.byref(dout), C.byref(k4.CultsCaps(cap_k, cap_d)), C.byref(tot2), None) == 0
    assert (tot2.n_located, tot2.n_kmers, tot2.n_dist, tot2.next_sfx_idx) == (tot.n_located, nk, nd, tot.next_sfx_idx)
    back = np.zeros(nk * 32, dtype=np.uint8)
    assert L.k4_copy_to_host(ix.h, back.ctypes.data, d[0], nk * 32) == 0 and np.array_equal(back, kmers[:nk * 32])
    for ptr in d:
        L.k4_free_device(ptr)
    # caps the call refuses
    for ck, cd in ((0, 40), (7, 4)):
        assert L.k4_kmer_cults_batch(ix.h, C.byref(p), 0, 0, C.byref(out), C.byref(k4.CultsCaps(ck, cd)), C.byref(tot)) == -100


def test_sfx_els_and_thread_range(k4, ix, crafted):
    seq, sa, _ = crafted[1]
    n = len(sa)
    assert ix.sfx_els(0, 50).tolist() == sa[:50] and ix.sfx_els(n - 3, 3).tolist() == sa[-3:]
    with pytest.raises(k4.K4Error):
        ix.sfx_els(n - 1, 2)
    for nt in (1, 2, 4):
        start = 0
        for t in range(1, nt + 1):
            got = ix.kmer_cult_thread_range(cc.P, t, nt, start)
            assert got == cults_ref.thread_range(crafted[1], cc.P, t, nt, start), (nt, t)
            start = got[1] + 1
    assert ix.kmer_cult_thread_range(cc.P, 0, 2, 0)[0] == -1 and ix.kmer_cult_thread_range(cc.P, 1, 65, 0)[0] == -1


@pytest.fixture(scope="module")
def built(k4, oracle):
    made = []

    def make(names, chroms, el):
        h = oracle.build(names, chroms, dataset="c", force_el=el if el == 5 else 0, threads=4)
        cat = oracle.concat_len(h)
        sa_raw = np.ctypeslib.as_array(C.cast(oracle.L.k4o_sa_bytes(h), C.POINTER(C.c_uint8)), shape=(cat * el,))
        x = k4.SfxIndex.from_host(np.array(oracle.seq(h)), sa_raw, el, k4.make_entries(names, [len(c) for c in chroms]), dataset="c")
        made.append((x, h))
        return x, query_ref.index_from_oracle(oracle, h)

    yield make
    for x, h in made:
        x.close()
        oracle.close(h)


def _family(n, length=90, seed=3, muts=3):
    """n cultivars of `length` bases that descend from one ancestor by muts substitutions each, every fifth reverse complemented"""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, length).astype(np.uint8)
    out = []
    for i in range(n):
        a = anc.copy()
        for p in rng.choice(length, muts, replace=False):
            a[p] = (a[p] + 1 + rng.integers(0, 3)) % 4
        out.append(query_ref.revcomp(a) if i % 5 == 4 else a)
    return ["c%d" % i for i in range(n)], out


@pytest.mark.parametrize("n_targets", [129, 300])
def test_more_than_128_targets(k4, built, n_targets):
    """the entry table is searched in global memory; counts over hundreds of entries"""
    names, chroms = mt.small_genome(n_targets)
    _, fam = _family(n_targets)
    chroms = [np.concatenate([c, f]) for c, f in zip(chroms, fam)]
    x, ref = built(names, chroms, 4)
    for kw in (dict(plen=14, slen=4, min_cult=n_targets // 3), dict(plen=10, slen=0, min_cult=2)):
        rc, recs = cults_ref.gen_kmer_cults_cnts(ref, False, 0, 0, kw["plen"], kw["slen"], kw["min_cult"])
        assert recs and max(len(r["cult"]) for r in recs) > 64
        got = x.kmer_cults(kw["plen"], kw["slen"], kw["min_cult"], max_window=4096)
        _same(k4, got, rc, recs, kw["plen"] + kw["slen"], (n_targets, kw))


@pytest.mark.parametrize("n_targets", [2048, 2049])
def test_both_sides_of_the_lds_histogram_bound(k4, built, n_targets):
    """2048 entries count in LDS, 2049 in the global slices: the same family of short cultivars on each side"""
    names, fam = _family(n_targets, length=30, seed=9, muts=1)
    x, ref = built(names, fam, 4)
    rc, recs = cults_ref.gen_kmer_cults_cnts(ref, False, 0, 0, 12, 2, 40)
    assert len(recs) > 10 and max(len(r["cult"]) for r in recs) > 500
    _same(k4, x.kmer_cults(12, 2, 40, max_window=8192, max_kmers=256, max_dist=4 * n_targets), rc, recs, 14, n_targets)


def test_five_byte_suffix_elements(k4, built, crafted, golden_dir):
    names, ts = cc.targets()
    x, ref = built(names, ts, 5)
    assert x.info()["sfx_el_size"] == 5
    n = len(ref[1])
    assert x.sfx_els(0, 70).tolist() == ref[1][:70] and x.sfx_els(n - 5, 5).tolist() == ref[1][-5:] and x.sfx_els(1001, 3).tolist() == ref[1][1001:1004]
    for name in ("min1", "sense_only_min1", "p20_s4_min2"):
        kw = [c for c in cc.cases() if c[0] == name][0][1]
        rc, recs = cults_ref.gen_kmer_cults_cnts(ref, kw["sense_only"], 0, 0, kw["plen"], kw["slen"], kw["min_cult"])
        _same(k4, _call(x, kw, (0, 0), max_window=64), rc, recs, kw["plen"] + kw["slen"], name)


def _facade(sfx, tmp_path, tag, blob, located, abort_blob, min_cult, threads):
    exe = os.path.join(ROOT, "kit4b_amd", "k4_cults_facade_test")
    assert os.path.exists(exe), "make -C kit4b_amd/csrc"
    f = tmp_path / (tag + ".bin")
    f.write_bytes(bytes(blob))
    ab = "-"
    if abort_blob is not None:
        ab = str(tmp_path / (tag + "_abort.bin"))
        open(ab, "wb").write(bytes(abort_blob))
    out = subprocess.run([exe, sfx, str(f), str(located), ab, str(min_cult), str(threads)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def test_csfxarray_cults_facade_program(crafted, golden_dir, tmp_path):
    """CSfxArray::GenKMerCultThreadRange / GenKMerCultsCnts of include/k4_sfxarray.hpp on the crafted index, partitioned for four
    threads (which leaves one active: the index is short): the callbacks (dense tsKMerCultsCnts) are the golden's, an aborting
    callback ends the call with its value, the parameter errors and the unsupported call"""
    g = load_cases(golden_dir)
    i = [c[0] for c in cc.cases()].index("min1")
    got = _facade(crafted[0], tmp_path, "min1", g["cb_%d" % i], int(g["rc"][i]), g["abort_cb"], 1, 4)
    assert got == ["threads 4 active 1 located %d callbacks match" % int(g["rc"][i]), "abort -7 after 3 match", "errors -1 -1 -1 unsupported -3"], got


@pytest.fixture(scope="module")
def big(k4, oracle, tmp_path_factory):
    """the large cultivar set as a .sfx file from the project's builder, opened on the device"""
    names, ts = cc.big_targets()
    h = oracle.build(names, ts, dataset="cultsbig", threads=4)
    p = str(tmp_path_factory.mktemp("cultsbig") / "cults_big.sfx")
    oracle.write(h, p)
    oracle.close(h)
    x = k4.SfxIndex.open(p)
    yield p, x
    x.close()


def test_big_thread_ranges_on_the_device_index(k4, big, golden_dir):
    """SfxIndex.kmer_cult_thread_range where the search for a boundary runs: the reference's ranges for 2, 3 and 4 threads"""
    g = load_big(golden_dir)
    want = [tuple(int(v) for v in row) for row in g["tr"]]
    rng = lambda _, klen, t, nt, start: big[1].kmer_cult_thread_range(klen, t, nt, start)
    assert [(nt,) + r for nt in cc.BIG_THREADS for r in cc.thread_ranges(None, rng, nt)] == want


@pytest.mark.parametrize("threads", [3, 4])
def test_big_facade_program_with_concurrent_threads(big, golden_dir, tmp_path, threads):
    """every thread of the partition is active and sweeps its range at the same time as the others, through one CSfxArray; three
    threads cut two K-mers off their other elements, which both neighbours then hand to the callback"""
    g = load_big(golden_dir)
    located = int(g["located%d" % threads].sum())
    got = _facade(big[0], tmp_path, "big%d" % threads, g["cb_all%d" % threads], located, None, 0, threads)
    assert got == ["threads %d active %d located %d callbacks match" % (threads, threads, located)], got


def test_big_kmermarkers_fasta_and_small_caps(k4, oracle, big, golden_dir):
    """the front end's file with four threads from the device sweep; and the sweep with room for 100 K-mers per call, which cuts its
    windows down to that room, equals the restatement"""
    import lzma

    with lzma.open(os.path.join(golden_dir, "cults_big_k20_T4.fa.xz"), "rb") as f:
        want = f.read().decode()
    assert fasta_records(k4.kmermarkers_fasta(big[1], 20, threads=4).splitlines()) == fasta_records(want.splitlines())
    ref = big_index(oracle)
    rc, recs = cults_ref.gen_kmer_cults_cnts(ref, False, 0, 0, cc.P, cc.S, 0)
    _same(k4, big[1].kmer_cults(cc.P, cc.S, 0, max_kmers=100, max_dist=700), rc, recs, cc.P + cc.S, "small caps")
    _same(k4, big[1].kmer_cults(cc.P, cc.S, 0), rc, recs, cc.P + cc.S, "default caps")
