"""Restricted Hammings on the device (k4_hamming.hip) through the C ABI, the Python binding and the C++ facade: the reference's own
bytes (tests/golden/hamm_*.xz, the front end's CSV files and logged distribution) and, on fresh inputs, the Python restatement that
test_hamm_cpu.py pins to them.  Every byte is compared, the ones no K-mer owns included."""
import ctypes as C
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import blitz_ref
import hamm_craft as hc
import hamm_ref
import manytargets as mt
import query_ref
import runlen_craft as rc
from test_hamm_cpu import distribution, load_cases, load_run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


@pytest.fixture(scope="module")
def sfx_path(golden_dir, tmp_path_factory):
    p = tmp_path_factory.mktemp("hamm") / "hamm_index.sfx"
    with lzma.open(os.path.join(golden_dir, "hamm_index.sfx.xz"), "rb") as f:
        p.write_bytes(f.read())
    return str(p)


@pytest.fixture(scope="module")
def ix(k4, sfx_path):
    x = k4.SfxIndex.open(sfx_path)
    yield x
    x.close()


@pytest.fixture(scope="module")
def ref_index(oracle, sfx_path):
    h = oracle.open(sfx_path)
    yield query_ref.index_from_oracle(oracle, h)
    oracle.close(h)


def _kw(p):
    rhamm, both, nth, mn, mx, iib = p
    return dict(rhamm=rhamm, both_strands=bool(both), sample_nth=nth, min_core_depth=mn, max_core_depth=mx, intra_inter_both=iib)


def test_python_methods_return_the_reference_bytes(ix, golden_dir):
    """every crafted case, one call each: stages, copies and filters, N, boundaries, depth caps, sampling, outside sequences"""
    g = load_cases(golden_dir)
    for i, (name, form, what, p, _) in enumerate(hc.cases()):
        got = ix.sfx_hammings([what], hc.K, **_kw(p))[0] if form == "sfx" else ix.hammings([what], hc.K, **_kw(p))[0]
        assert got.dtype == np.uint8 and np.array_equal(got, g["out_%d" % i]), (name, got[:16], g["out_%d" % i][:16])


def _by_params(cases, form):
    by = {}
    for i, c in enumerate(cases):
        if c[1] == form:
            by.setdefault(c[3], []).append(i)
    return by


def test_c_abi_batch_and_dev_entry_points(k4, ix, golden_dir):
    """k4_locate_[sfx_]hammings_batch and _batch_dev themselves: the cases of one parameter set as one batch into one array with
    gaps between the spans; the gaps and the bytes behind the last K-mer of a span keep the caller's fill"""
    g = load_cases(golden_dir)
    cases = hc.cases()
    L = k4.lib()
    for form in ("sfx", "seq"):
        for p, idx in _by_params(cases, form).items():
            n = len(idx)
            lens = np.array([cases[i][2][2] if form == "sfx" else len(cases[i][2]) for i in idx], dtype=np.uint32)
            out_offs = (np.concatenate([[0], np.cumsum(lens[:-1] + 5)]) + 3).astype(np.uint64)
            total = int(out_offs[-1] + lens[-1]) + 7
            want = np.full(total, 0xEE, dtype=np.uint8)
            for k, i in enumerate(idx):
                w = g["out_%d" % i]
                seg = want[int(out_offs[k]):int(out_offs[k]) + len(w)]
                seg[w != 0xFF] = w[w != 0xFF]
            hp = k4.HammingParams(p[0], hc.K, p[2], p[1], p[3], p[4], p[5])
            host = np.full(total, 0xEE, dtype=np.uint8)
            d_out = C.c_void_p()
            assert L.k4_alloc_device(ix.h, total, C.byref(d_out)) == 0
            assert L.k4_copy_to_device(ix.h, d_out, host.ctypes.data, total) == 0
            dev = np.zeros(total, dtype=np.uint8)
            if form == "sfx":
                ids, locis = (np.array([cases[i][2][k] for i in idx], dtype=np.uint32) for k in (0, 1))
                args = (ix.h, C.byref(hp), n, ids.ctypes.data, locis.ctypes.data, lens.ctypes.data, out_offs.ctypes.data)
                assert L.k4_locate_sfx_hammings_batch(*args, host.ctypes.data, total) == 0
                assert L.k4_locate_sfx_hammings_batch_dev(*args, d_out, total, None) == 0
            else:
                cat, offs, _ = k4._flatten([np.ascontiguousarray(cases[i][2]) for i in idx])
                cat = np.concatenate([cat, np.zeros(16, np.uint8)])
                d_cat = C.c_void_p()
                assert L.k4_alloc_device(ix.h, len(cat), C.byref(d_cat)) == 0
                assert L.k4_copy_to_device(ix.h, d_cat, cat.ctypes.data, len(cat)) == 0
                tail = (offs.ctypes.data, lens.ctypes.data, out_offs.ctypes.data)
                assert L.k4_locate_hammings_batch(ix.h, C.byref(hp), n, cat.ctypes.data, *tail, host.ctypes.data, total) == 0
                assert L.k4_locate_hammings_batch_dev(ix.h, C.byref(hp), n, d_cat, *tail, d_out, total, None) == 0
                L.k4_free_device(d_cat)
            assert L.k4_copy_to_host(ix.h, dev.ctypes.data, d_out, total) == 0
            L.k4_free_device(d_out)
            assert np.array_equal(host, want), (form, p, np.nonzero(host != want)[0][:8])
            assert np.array_equal(dev, want), (form, p, np.nonzero(dev != want)[0][:8])
    assert L.k4_hamming_last_kernel_ms(ix.h) > 0


@pytest.mark.parametrize("run,kw", hc.CSV_RUNS)
def test_restricted_hammings_and_report_reproduce_the_front_end(k4, ix, golden_dir, run, kw):
    """the whole index at the default preset: the bytes the reference's engine calls left, and its front end's CSV file (its
    logged distribution for the sampled run, which writes no file)"""
    names, ts = hc.targets()
    lens = [len(t) for t in ts]
    got = ix.restricted_hammings(**kw)
    assert np.array_equal(got, load_run(golden_dir, run)), np.nonzero(got != load_run(golden_dir, run))[0][:8]
    if kw.get("sample_nth", 1) == 1:
        with lzma.open(os.path.join(golden_dir, run + ".csv.xz"), "rb") as f:
            assert k4.hammings_csv(names, lens, got, kw["kmer_len"]) == f.read().decode()
    else:
        assert distribution(lens, got, kw["kmer_len"], kw["rhamm"]) == json.load(open(os.path.join(golden_dir, run + ".dist.json")))


def _restate(ref, spans, klen, p, n_out, out_offs):
    want = np.full(n_out, 0xFF, dtype=np.uint8)
    for (eid, loci, sl), o in zip(spans, out_offs):
        assert hamm_ref.locate_sfx_hammings(ref, p[0], bool(p[1]), klen, p[2], sl, p[3], p[4], eid, loci, p[5], want, int(o)) == 0
    return want


def test_mixed_batch_equals_the_restatement(k4, ix, ref_index):
    """spans of K, K + 1 and a few hundred bases over all four targets in one batch, sampled and on both strands, at K = 40; an
    empty batch writes nothing; a span shorter than K (an empty one too) fails the call as it fails the reference's, alone or
    among good ones, and nothing is written"""
    klen, p = 40, (3, 1, 2, 2, 3, 0)
    spans = [(1, 180, klen), (2, 490, klen + 1), (3, 1380, 130), (4, 5990, 90), (1, 3000 - klen, klen), (4, 0, 45), (2, 1940, 60)]
    lens = [s[2] for s in spans]
    out_offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    got = ix.sfx_hammings(spans, klen, **_kw(p))
    want = _restate(ref_index, spans, klen, p, sum(lens), out_offs)
    assert np.array_equal(np.concatenate(got), want), np.nonzero(np.concatenate(got) != want)[0][:8]
    assert len({int(v) for v in want}) >= 4
    assert ix.sfx_hammings([], klen, **_kw(p)) == []
    out = np.full(64, 0xAB, dtype=np.uint8)
    for bad in ([(1, 0, 0)], [(1, 0, klen - 1)], [(1, 0, klen), (2, 5, klen - 1)]):
        assert hamm_ref.locate_sfx_hammings(ref_index, p[0], True, klen, p[2], bad[-1][2], p[3], p[4], bad[-1][0], bad[-1][1], 0,
                                            np.zeros(64, np.uint8)) == hamm_ref.ERR_INTERNAL
        with pytest.raises(k4.K4Error) as e:
            ix.sfx_hammings(bad, klen, out=out, out_offs=np.zeros(len(bad), np.uint64), **_kw(p))
        assert e.value.code == -1
    assert (out == 0xAB).all()


def test_host_pointer_calls_of_the_three_families_share_their_staging(k4, sfx_path, ref_index):
    """on a fresh handle: LocateHammings over a short batch, LocateQuerySeqs, blitz's path stage, LocateHammings over a longer batch
    (the staged batch grows): each the restatement's answer, so no family reads what another left in the shared buffers; then each
    family's device time is 0 behind a batch of nothing"""
    _, ts = hc.targets()
    klen, rhamm, mn, mx = 24, 2, 3, 4
    x = k4.SfxIndex.open(sfx_path)
    try:
        def hamm(seqs):
            got = x.hammings(seqs, klen, rhamm, mn, mx, both_strands=True)
            for s, g in zip(seqs, got):
                want = np.full(len(s), 0xFF, dtype=np.uint8)
                assert hamm_ref.locate_hammings(ref_index, rhamm, True, klen, 1, s, mn, mx, 0, want) == 0
                assert np.array_equal(g, want), (len(s), g, want)
            return got

        near = ts[0][400:400 + klen + 3].copy()
        near[5] = (near[5] + 1) % 4
        short = hamm([near, ts[2][50:50 + klen + 3].copy()])
        assert int(short[0][0]) == 1 and int(short[1][0]) == 0 and x.hamming_kernel_ms() > 0
        qs = [ts[1][100:400].copy(), query_ref.revcomp(ts[3][700:900]), ts[0][2000:2090].copy()]
        lp = (20, 10, 0, 1000, 100, 1, 3)
        nodes = x.locate_query_seqs(qs, *lp)
        want_nodes = [query_ref.locate_query_seqs(ref_index, q, *lp) for q in qs]
        assert [[tuple(int(r[f]) for f in query_ref.NODE_FIELDS) for r in a] for a in nodes] == want_nodes and all(want_nodes)
        assert x.query_kernel_ms() > 0
        path_offs, paths, blocks = x.blitz_paths(qs, None, nodes)
        want_paths, want_blocks = [], []
        for i, q in enumerate(qs):
            ps, bs = blitz_ref.blitz_paths(ref_index, q, want_nodes[i], query_idx=i)
            want_paths += [p[:16] + (p[16] + len(want_blocks),) for p in ps]
            want_blocks += bs
        assert [tuple(int(r[f]) for f in blitz_ref.PATH_FIELDS) for r in paths] == want_paths and len(want_paths) == len(qs)
        assert [tuple(int(r[f]) for f in blitz_ref.BLOCK_FIELDS) for r in blocks] == want_blocks
        assert [int(v) for v in path_offs] == [0, 1, 2, 3] and k4.lib().k4_blitz_last_kernel_ms(x.h) > 0
        far = ts[3][3000:3120].copy()
        far[::7] = (far[::7] + 2) % 4
        hamm([ts[0][280:400].copy(), far, ts[1][1900:2000].copy(), near])
        assert x.hammings([], klen, rhamm, mn, mx) == [] and x.hamming_kernel_ms() == 0
        assert x.locate_query_seqs([], *lp) == [] and x.query_kernel_ms() == 0
        assert len(x.blitz_paths([], None, [])[1]) == 0 and k4.lib().k4_blitz_last_kernel_ms(x.h) == 0
    finally:
        x.close()


def test_parameter_errors(k4, ix):
    out = np.full(200, 0xCD, dtype=np.uint8)

    def call(spans=((1, 0, 60),), klen=60, rhamm=3, iib=0, offs=(0,), n_out=200):
        with pytest.raises(k4.K4Error) as e:
            ix.sfx_hammings(list(spans), klen, rhamm, 3, 4, intra_inter_both=iib, out=out[:n_out], out_offs=np.array(offs, dtype=np.uint64))
        return e.value.code

    assert call(spans=[(0, 0, 60)]) == -1 and call(spans=[(5, 0, 60)]) == -1     # entry 0, no such entry
    assert call(spans=[(1, 2941, 60)]) == -1 and call(spans=[(1, 3001, 60)]) == -1  # leaves its entry
    assert call(spans=[(1, 0, 59)]) == -1 and call(rhamm=0) == -1 and call(klen=9, spans=[(1, 0, 9)]) == -1
    assert call(klen=501, spans=[(1, 0, 600)]) == -1
    assert call(rhamm=11, klen=100, spans=[(1, 0, 100)]) == -100 and call(rhamm=7) == -100  # 60 / 8 = 7: a core under 8 bases
    assert b"core under 8" in k4.lib().k4_last_error(ix.h)
    assert call(iib=3) == -100
    assert call(spans=[(1, 0, 100)], n_out=40) == -100 and call(offs=(200,)) == -100  # the span's bytes leave the array
    assert (out == 0xCD).all()
    with pytest.raises(k4.K4Error) as e:
        ix.hammings([np.zeros(59, np.uint8)], 60, 3, 3, 4)
    assert e.value.code == -1


@pytest.fixture(scope="module")
def built(k4, oracle):
    made = []

    def make(names, chroms, el):
        h = oracle.build(names, chroms, dataset="h", force_el=el if el == 5 else 0, threads=4)
        cat = oracle.concat_len(h)
        sa_raw = np.ctypeslib.as_array(C.cast(oracle.L.k4o_sa_bytes(h), C.POINTER(C.c_uint8)), shape=(cat * el,))
        x = k4.SfxIndex.from_host(np.array(oracle.seq(h)), sa_raw, el, k4.make_entries(names, [len(c) for c in chroms]), dataset="h")
        made.append((x, h))
        return x, query_ref.index_from_oracle(oracle, h)

    yield make
    for x, h in made:
        x.close()
        oracle.close(h)


def test_more_than_128_targets(built):
    """260 targets (the entry table is searched in global memory): K-mers of targets 4, 132 and 260, with an exact copy and a near
    copy planted across targets, under the three filters"""
    names, chroms = mt.small_genome(260)
    chroms = [c.copy() for c in chroms]
    chroms[3] = np.random.default_rng(5).integers(0, 4, 300).astype(np.uint8)
    klen = 40
    chroms[131][50:50 + klen] = chroms[3][20:20 + klen]
    near = chroms[3][100:100 + klen].copy()
    near[[7, 30]] = (near[[7, 30]] + 1) % 4
    chroms[259][10:10 + klen] = near
    x, ref = built(names, chroms, 4)
    spans = [(4, 15, 50), (132, 45, 50), (260, 5, 50), (4, 95, 50)]
    lens = [s[2] for s in spans]
    out_offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    for iib in (0, 1, 2):
        p = (3, 1, 1, 2, 3, iib)
        got = np.concatenate(x.sfx_hammings(spans, klen, **_kw(p)))
        assert np.array_equal(got, _restate(ref, spans, klen, p, sum(lens), out_offs)), iib
        assert int(got[5]) == (0 if iib != 1 else 4) and int(got[150 + 5]) == 2


def test_five_byte_suffix_elements(built, golden_dir):
    """the crafted targets indexed with 5-byte elements: the single-K-mer cases as the reference answered them.  (The depth cases
    hold no tie through an end-of-sequence symbol inside a capped run, so the builder's order of such ties does not matter.)"""
    names, ts = hc.targets()
    x, _ = built(names, ts, 5)
    assert x.info()["sfx_el_size"] == 5
    g = load_cases(golden_dir)
    for i, (name, form, what, p, expect) in enumerate(hc.cases()):
        if form == "sfx" and expect:
            assert np.array_equal(x.sfx_hammings([what], hc.K, **_kw(p))[0], g["out_%d" % i]), name


def test_a_span_that_crosses_a_launch_window(k4, oracle):
    """runlen_craft.hamming_window(): one sfx span of 32 768 + 213 K-mers of 20 (rhamm 1, every K-mer, depths 1 / 10) takes two
    launches.  The same bytes as two calls whose spans meet at K-mer 20 000, neither of which leaves one launch; and the
    restatement's on the 128 K-mers around K-mer 32 768."""
    names, chroms = rc.hamming_window()
    klen, p, n = 20, (1, 0, 1, 1, 10, 0), 33000
    with rc.host_index(k4, oracle, names, chroms, dataset="hwin") as (x, ref):
        whole = x.sfx_hammings([(1, 0, n)], klen, **_kw(p))[0]
        assert x.hamming_kernel_ms() > 0
        parts = np.full(n, 0xFF, dtype=np.uint8)
        x.sfx_hammings([(1, 0, 20000 + klen - 1)], klen, out=parts, out_offs=[0], **_kw(p))
        x.sfx_hammings([(1, 20000, n - 20000)], klen, out=parts, out_offs=[20000], **_kw(p))
        assert np.array_equal(whole, parts), np.nonzero(whole != parts)[0][:8]
        assert (whole[:n - klen + 1] != 0xFF).all() and (whole[n - klen + 1:] == 0xFF).all()
        lo = 32768 - 64
        want = _restate(ref, [(1, lo, 128 + klen - 1)], klen, p, 128 + klen - 1, [0])[:128]
        assert np.array_equal(whole[lo:lo + 128], want), (whole[lo:lo + 128].tolist(), want.tolist())
        assert len(set(want[:64].tolist())) >= 2 and len(set(want[64:].tolist())) >= 2


def test_csfxarray_hamming_facade_program(sfx_path, golden_dir, tmp_path):
    """eight threads call CSfxArray::LocateSfxHammings / LocateHammings of include/k4_sfxarray.hpp at once, each asking for
    different spans: every byte of every answer is the fixture's; then the reference's return codes for bad spans"""
    exe = os.path.join(ROOT, "kit4b_amd", "k4_hamming_facade_test")
    assert os.path.exists(exe), "make -C kit4b_amd/csrc"
    g = load_cases(golden_dir)
    lines = []
    cases = hc.cases()
    for i, (name, form, what, p, _) in enumerate(cases):
        rhamm, both, nth, mn, mx, iib = p
        w = g["out_%d" % i]
        ent, loci = (what[0], what[1]) if form == "sfx" else (0, 0)
        lines.append(" ".join(str(v) for v in (0 if form == "sfx" else 1, rhamm, both, hc.K, nth, mn, mx, iib, ent, loci, len(w))))
        if form == "seq":
            lines.append("".join(str(int(b)) for b in what))
        lines.append(" ".join(str(int(v)) for v in w))
    f = tmp_path / "cases.txt"
    f.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, sfx_path, str(f)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    o = out.stdout.splitlines()
    assert o[0] == "threads 8 cases %d bad 0 msgs 0" % len(cases), out.stdout
    assert o[1:] == ["entry 0 -> -1", "short span -> -1", "past entry -> -1", "core under 8 -> -100 msgs 2", "untouched 1"], out.stdout
