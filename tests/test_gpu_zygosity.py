"""genzygosity on the device (k4_zygosity.hip) through the C ABI, the Python binding and the C++ facade: LocateAllNearMatches
against the reference's recorded returns, the scan against the Python restatement that test_zygosity_cpu.py pins to those
recordings, and genzygosity_csv against the front end's recorded files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cults_craft as cc
import query_ref
import runlen_craft as rc
import zyg_craft as zc
import zyg_ref as zr
from test_cults_cpu import big_index
from test_zygosity_cpu import COLS, call_list, golden_file, load_calls, load_index, scan_kw, scan_results

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTALS = ("windows", "passed_over", "rejected", "unique", "unique_matched", "ordered")
LIMITS = ("max_tot_mm", "core_len", "core_delta", "max_core_slides", "max_matches", "cur_max_iter", "n_ident_nodes")


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


def groups_of(calls):
    """the recorded calls by their limits: one device batch each"""
    g = {}
    for i, c in enumerate(calls):
        g.setdefault(tuple(c[k] for k in LIMITS), []).append(i)
    return g


def test_all_near_matches_equal_the_recorded_returns(ix, golden_dir):
    calls = call_list(load_calls(golden_dir))
    for lim, members in groups_of(calls).items():
        rs, cnt = ix.all_near_matches([calls[i]["probe"] for i in members], [calls[i]["probe_entry"] for i in members],
                                      [calls[i]["probe_ofs"] for i in members], **dict(zip(LIMITS, lim)))
        assert ix.zygosity_kernel_ms() > 0
        for r, row, i in zip(rs, cnt, members):
            c = calls[i]
            assert int(r) == c["rslt"] and row[:c["num_entries"]].tolist() == c["cnt"], (i, int(r), c["rslt"], row.tolist(), c["cnt"])
        rs2, none = ix.all_near_matches([calls[i]["probe"] for i in members], [calls[i]["probe_entry"] for i in members],
                                        [calls[i]["probe_ofs"] for i in members], counts=False, **dict(zip(LIMITS, lim)))
        assert none is None and np.array_equal(rs, rs2)
    r0, c0 = ix.all_near_matches([], [], [], 2, 9, 9, 4)
    assert len(r0) == 0 and ix.zygosity_kernel_ms() == 0


def test_the_ordered_walk_beyond_the_table_in_lds(ix, crafted):
    """windows of 50 bases in and at the edge of zE's (AC)n stretch, asked as if they came from zD: five cores of 10, each a run of
    some 1200 suffixes, MaxIter 1000 -- up to 5000 ids a pass, more than the LDS table's 1024: the probes go to the second launch
    and answer as the restatement does, in a batch and alone"""
    names, seqs, sites = zc.build()
    at = seqs[4].tobytes().find(bytes([0, 1] * 15))
    ofs = [at - 30, at - 7, at, at + 1, at + 200]
    probes = [seqs[4][o:o + 50] for o in ofs]
    most = 0
    for it, mx in ((1000, 0), (1000, 3), (300, 0), (0, 0), (0, 3)):
        want = [zr.near_matches(crafted[1], 4, 10, 10, 8, mx, 8, 4, o, p.tobytes(), it, zr.NODES) for p, o in zip(probes, ofs)]
        n_ord = sum(zr.needs_ordered_walk(crafted[1], p.tobytes(), 10, 10, 8, it, zr.NODES) for p in probes)
        assert n_ord >= 3 if it else n_ord == 0
        rs, cnt = ix.all_near_matches(probes, [4] * len(probes), ofs, 4, 10, 10, 8, max_matches=mx, cur_max_iter=it)
        assert rs.tolist() == [w[0] for w in want] and cnt.tolist() == [w[1] for w in want], (it, mx)
        one, cnt1 = ix.all_near_matches(probes[2:3], [4], ofs[2:3], 4, 10, 10, 8, max_matches=mx, cur_max_iter=it)
        assert int(one[0]) == want[2][0] and cnt1[0].tolist() == want[2][1]
        most = max(most, max(w[0] for w in want))
    assert most > 1000


def dev_near_matches(k4, ix, lim, probes, entries, ofs):
    """k4_all_near_matches_batch_dev on buffers of the caller's with 0xEE behind every output: (rslts, counts), the guards checked"""
    L = k4.lib()
    n, n_ent = len(probes), ix.info()["n_entries"]
    lens = np.array([len(p) for p in probes], dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    arrays = [np.concatenate(list(probes) + [np.zeros(16, np.uint8)]), offs, lens, np.array(entries, dtype=np.uint32), np.array(ofs, dtype=np.uint32),
              np.full(4 * (n + 2), 0xEE, np.uint8), np.full(4 * (n * n_ent + 8), 0xEE, np.uint8)]
    p = k4.NearParams(*lim, 0)
    d = [C.c_void_p() for _ in arrays]
    try:
        for ptr, a in zip(d, arrays):
            assert L.k4_alloc_device(ix.h, a.nbytes, C.byref(ptr)) == 0
            assert L.k4_copy_to_device(ix.h, ptr, a.ctypes.data, a.nbytes) == 0
        assert L.k4_all_near_matches_batch_dev(ix.h, C.byref(p), n, d[0], d[1], d[2], d[3], d[4], d[5], d[6], n * n_ent - 1, None) == zr.ERR_PARAMS
        assert ix.zygosity_kernel_ms() == 0
        assert L.k4_all_near_matches_batch_dev(ix.h, C.byref(p), n, d[0], d[1], d[2], d[3], d[4], d[5], d[6], n * n_ent, None) == 0
        assert ix.zygosity_kernel_ms() > 0
        for ptr, a in zip(d[5:], arrays[5:]):
            assert L.k4_copy_to_host(ix.h, a.ctypes.data, ptr, a.nbytes) == 0
    finally:
        for ptr in d:
            L.k4_free_device(ptr)
    assert (arrays[5][4 * n:] == 0xEE).all() and (arrays[6][4 * n * n_ent:] == 0xEE).all(), lim
    return arrays[5][:4 * n].view(np.int32), arrays[6][:4 * n * n_ent].view(np.uint32).reshape(n, n_ent)


def test_all_near_matches_dev_form_and_untouched_bytes(k4, ix, crafted, golden_dir):
    """every recorded call through the _dev form, one batch per set of limits, results and rows written into the caller's device
    buffers by whichever launch answers the probe; then the probes of the (AC)n stretch, whose rows the second launch writes"""
    calls = call_list(load_calls(golden_dir))
    n_ordered = n_minus = 0
    for lim, members in groups_of(calls).items():
        rs, cnt = dev_near_matches(k4, ix, lim, [calls[i]["probe"] for i in members], [calls[i]["probe_entry"] for i in members],
                                   [calls[i]["probe_ofs"] for i in members])
        for r, row, i in zip(rs, cnt, members):
            c = calls[i]
            assert int(r) == c["rslt"] and row[:c["num_entries"]].tolist() == c["cnt"], (i, int(r), c["rslt"], row.tolist(), c["cnt"])
            n_ordered += zr.needs_ordered_walk(crafted[1], c["probe"].tobytes(), c["core_len"], c["core_delta"], c["max_core_slides"], c["cur_max_iter"],
                                               c["n_ident_nodes"])
            n_minus += c["rslt"] < 0 and sum(c["cnt"]) > 0
    assert n_ordered >= 20 and n_minus >= 5
    names, seqs, sites = zc.build()
    at = seqs[4].tobytes().find(bytes([0, 1] * 15))
    ofs = [at - 30, at - 7, at, at + 1, at + 200]
    probes = [seqs[4][o:o + 50] for o in ofs]
    for it, mx in ((1000, 0), (1000, 3), (0, 3)):
        want = [zr.near_matches(crafted[1], 4, 10, 10, 8, mx, 8, 4, o, p.tobytes(), it, zr.NODES) for p, o in zip(probes, ofs)]
        rs, cnt = dev_near_matches(k4, ix, (4, 10, 10, 8, mx, it, zr.NODES), probes, [4] * len(probes), ofs)
        assert rs.tolist() == [w[0] for w in want] and cnt.tolist() == [w[1] for w in want], (it, mx)


@pytest.mark.parametrize("stem,kw", zc.scan_cases())
def test_zygosity_equals_the_restatement(k4, ix, crafted, golden_dir, stem, kw):
    m, s, tot, status = scan_results(crafted[1])[stem]
    gm, gs, gt, gst = ix.zygosity(status=True, **scan_kw(kw))
    assert ix.zygosity_kernel_ms() > 0
    assert np.array_equal(gst, status), np.flatnonzero(gst != status)[:5]
    assert np.array_equal(gm, m) and np.array_equal(gs, s) and [gt[k] for k in TOTALS] == [tot[k] for k in TOTALS]
    thr, raw = k4.genzygosity_csv(ix, **kw)
    assert thr == golden_file(golden_dir, stem + ".csv.xz") and raw == golden_file(golden_dir, stem + "_raw.csv.xz")


def test_the_second_launch_of_the_scan(ix, crafted):
    """-m3 (MaxIter 1000, cores of 11 at 0 and 11) inside the repeat families: both runs are cut at 1000, so a pass may hold 2000
    ids, more than the LDS table's 1024.  (At -m2 MaxIter is 50 000, more suffixes than this index has: no run is ever cut and
    no window leaves the unordered path, whatever the family's size.)"""
    stem, kw = zc.scan_cases()[1]
    gt = ix.zygosity(**scan_kw(kw))[2]
    assert gt["second_launch"] >= 1 and gt["ordered"] > gt["second_launch"]
    assert ix.zygosity(**scan_kw(zc.scan_cases()[2][1]))[2]["second_launch"] == 0


def test_windowed_scans_add_up(ix, crafted):
    m, s, tot, status = scan_results(crafted[1])["zygosity_l25_s2"]
    parts = [ix.zygosity(src_first=a, src_count=c, status=True) for a, c in ((1, 3), (4, 1), (5, 4))]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), m) and np.array_equal(np.concatenate([p[1] for p in parts]), s)
    assert np.array_equal(np.concatenate([p[3] for p in parts]), status)
    assert [sum(p[2][k] for p in parts) for k in TOTALS] == [tot[k] for k in TOTALS]
    e0 = ix.zygosity(src_first=3, src_count=0)
    assert e0[0].shape == (0, 8) and e0[2]["windows"] == 0 and ix.zygosity_kernel_ms() == 0


def test_status_bytes_behind_the_loci_stay(k4, ix, crafted):
    m, s, tot, status = scan_results(crafted[1])["zygosity_l25_s2"]
    L = k4.lib()
    n_ent, n = 8, len(status)
    p, t = k4.ZygosityParams(25, 2, 1, 5000, 0, 0), k4.ZygosityTotals()
    hm, hs, hst = np.full(n_ent * n_ent + 4, 0xEEEEEEEE, np.uint32), np.full(n_ent + 4, 0xEEEEEEEE, np.uint32), np.full(n + 64, 0xEE, np.uint8)
    assert L.k4_zygosity_batch(ix.h, C.byref(p), 1, n_ent, hm.ctypes.data, hs.ctypes.data, hst.ctypes.data, n - 1, C.byref(t)) == zr.ERR_PARAMS
    assert L.k4_zygosity_batch(ix.h, C.byref(p), 1, n_ent, hm.ctypes.data, hs.ctypes.data, hst.ctypes.data, n + 64, C.byref(t)) == 0
    assert np.array_equal(hm[:64].reshape(8, 8), m) and np.array_equal(hs[:8], s) and np.array_equal(hst[:n], status)
    assert (hm[64:] == 0xEEEEEEEE).all() and (hs[8:] == 0xEEEEEEEE).all() and (hst[n:] == 0xEE).all()
    arrays = [np.full(4 * (n_ent * n_ent + 4), 0xEE, np.uint8), np.full(4 * (n_ent + 4), 0xEE, np.uint8), np.full(n + 64, 0xEE, np.uint8)]
    d, t2 = [C.c_void_p() for _ in arrays], k4.ZygosityTotals()
    try:
        for ptr, a in zip(d, arrays):
            assert L.k4_alloc_device(ix.h, a.nbytes, C.byref(ptr)) == 0
            assert L.k4_copy_to_device(ix.h, ptr, a.ctypes.data, a.nbytes) == 0
        assert L.k4_zygosity_batch_dev(ix.h, C.byref(p), 1, n_ent, d[0], d[1], d[2], n + 64, C.byref(t2), None) == 0
        for ptr, a in zip(d, arrays):
            assert L.k4_copy_to_host(ix.h, a.ctypes.data, ptr, a.nbytes) == 0
    finally:
        for ptr in d:
            L.k4_free_device(ptr)
    assert np.array_equal(arrays[0].view(np.uint32), hm) and np.array_equal(arrays[1].view(np.uint32), hs) and np.array_equal(arrays[2], hst)
    assert [getattr(t2, k) for k in TOTALS] == [getattr(t, k) for k in TOTALS] == [tot[k] for k in TOTALS]


def test_a_second_index_on_the_same_file_answers_alike(k4, ix, crafted):
    """nothing was written into the index: an index opened after the first has run its scans answers alike"""
    m, s, tot, status = scan_results(crafted[1])["zygosity_l25_s2"]
    first = ix.zygosity(status=True)
    y = k4.SfxIndex.open(crafted[0])
    try:
        second = y.zygosity(status=True)
        for e in (1, 5):
            n = ix.entry(e)["seq_len"]
            assert np.array_equal(ix.get_seq(e, 0, n), y.get_seq(e, 0, n)) and int(ix.get_seq(e, 0, n).max()) <= 4  # no flag bits
    finally:
        y.close()
    for got in (first, second, ix.zygosity(status=True)):
        assert np.array_equal(got[0], m) and np.array_equal(got[1], s) and np.array_equal(got[3], status)


def test_parameter_errors(k4, ix):
    for kw in zc.error_cases():
        with pytest.raises(k4.K4Error) as e:
            ix.zygosity(**kw)
        assert e.value.code == zr.ERR_PARAMS, kw
        assert ix.zygosity_kernel_ms() == 0
    for ln, kw in zc.near_error_cases():
        with pytest.raises(k4.K4Error) as e:
            ix.all_near_matches([np.zeros(ln, np.uint8)], [1], [0], **kw)
        assert e.value.code == zr.ERR_PARAMS, (ln, kw)
        assert ix.zygosity_kernel_ms() == 0


def test_a_short_entry_has_a_zero_row(k4, oracle, tmp_path):
    names, seqs = zc.short_entry()
    h = oracle.build(names, seqs, dataset="zygshort", threads=2)
    p = tmp_path / "zygshort.sfx"
    oracle.write(h, str(p))
    ref = query_ref.index_from_oracle(oracle, h)
    oracle.close(h)
    m, s, tot, status = zr.zygosity(ref, 25, 2)
    x = k4.SfxIndex.open(str(p))
    try:
        gm, gs, gt, gst = x.zygosity(status=True)
    finally:
        x.close()
    assert np.array_equal(gm, m) and np.array_equal(gs, s) and np.array_equal(gst, status) and not gm[1].any() and gm[0, 2] > 0
    assert [gt[k] for k in TOTALS] == [tot[k] for k in TOTALS]


def test_big_targets_past_one_launch(k4, oracle, tmp_path_factory):
    """cults_craft.big_targets(): 6 x 17 000 bases 3 % apart; two source entries, 34 000 start loci at -l25 -s2 -- three launches
    of the scan (16 384 waves each).  -x4: a window that meets all five other cultivars is given up, so every status occurs (0 only
    where no window starts: the index holds no N)"""
    names, ts = cc.big_targets()
    h = oracle.build(names, ts, dataset="cultsbig", threads=4)
    p = tmp_path_factory.mktemp("zygbig") / "zygosity_big.sfx"
    oracle.write(h, str(p))
    oracle.close(h)
    m, s, tot, status = zr.zygosity(big_index(oracle), 25, 2, max_matches=4, src_first=2, src_count=2)
    x = k4.SfxIndex.open(str(p))
    try:
        gm, gs, gt, gst = x.zygosity(max_matches=4, src_first=2, src_count=2, status=True)
    finally:
        x.close()
    assert len(gst) == 34000 and np.array_equal(gst, status) and np.array_equal(gm, m) and np.array_equal(gs, s)
    assert [gt[k] for k in TOTALS] == [tot[k] for k in TOTALS]
    for launch in (gst[:16384], gst[16384:32768], gst[32768:]):
        assert (launch == 3).any() and (launch == 1).any()
    assert set(np.unique(gst)) == {0, 1, 2, 3} and gt["windows"] == 2 * (17000 - 24)


@pytest.mark.parametrize("r", (63, 64, 65, 129))
def test_runs_that_end_at_a_turn_of_the_walk(k4, oracle, r):
    """runlen_craft.zygosity_runs(r): a 25-base probe whose first core of 12 has exactly r occurrences, so the walk of that run
    ends one short of, at and one past a turn of 64 suffixes.  MaxMatches 0 and r - 1, CurMaxIter off, below r (the ordered walk,
    cut inside a turn) and above r (the unordered one), with and without substitutions allowed: the returns and the counts rows of
    the restatement."""
    names, chroms, probe, ofs = rc.zygosity_runs(r)
    with rc.host_index(k4, oracle, names, chroms) as (x, ref):
        assert x.exact_ranges([probe[:12]])[1].tolist() == [r]
        other = chroms[0][100:125]
        rslts = set()
        for mm in (2, 0):
            for mx in (0, r - 1, r // 2):  # (the last: given up inside a turn)
                for it in (0, r - 10, r + 10):
                    want = [zr.near_matches(ref, mm, 12, 12, 2, mx, 4, 1, o, p.tobytes(), it, zr.NODES) for p, o in ((probe, ofs), (other, 100))]
                    assert zr.needs_ordered_walk(ref, probe.tobytes(), 12, 12, 2, it, zr.NODES) == (it == r - 10)
                    rs, cnt = x.all_near_matches([probe, other], [1, 1], [ofs, 100], mm, 12, 12, 2, max_matches=mx, cur_max_iter=it)
                    assert rs.tolist() == [w[0] for w in want] and cnt.tolist() == [w[1] for w in want], (r, mm, mx, it, rs.tolist(), want[0][0])
                    rslts.add(want[0][0])
        assert max(rslts) == r - 1 and min(rslts) == -1 and len(rslts) >= 4


def test_csfxarray_zygosity_facade_program(crafted, golden_dir, tmp_path):
    """CSfxArray::LocateAllNearMatches for a third of the recorded calls and ZygosityBatch of include/k4_sfxarray.hpp"""
    exe = os.path.join(ROOT, "kit4b_amd", "k4_zygosity_facade_test")
    assert os.path.exists(exe), "make -C kit4b_amd/csrc"
    calls = call_list(load_calls(golden_dir))[::3]
    lines = []
    for c in calls:
        lines.append("%d %s %s %d %d %d %s" % (len(c["probe"]), "".join(str(int(b)) for b in c["probe"]), " ".join(str(c[k]) for k in COLS), c["cur_max_iter"],
                                              c["n_ident_nodes"], c["rslt"], " ".join(map(str, c["cnt"]))))
    (tmp_path / "calls.txt").write_text("\n".join(lines) + "\n")
    stem, kw = zc.scan_cases()[1]
    m, s, tot, status = scan_results(crafted[1])[stem]
    kw = dict(dict(max_ns=1, max_matches=5000, mode=0), **scan_kw(kw))
    (tmp_path / "scan.txt").write_text("%d %d %d %d %d %d\n%s\n%s\n%s %d\n%s\n" % (
        kw["subseq_len"], kw["max_subs"], kw["max_ns"], kw["max_matches"], kw["mode"], len(s), " ".join(map(str, s.tolist())),
        " ".join(map(str, m.ravel().tolist())), " ".join(str(tot[k]) for k in TOTALS[:5]), len(status), "".join(str(c) for c in status)))
    out = subprocess.run([exe, crafted[0], str(tmp_path / "calls.txt"), str(tmp_path / "scan.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines() == ["calls %d bad returns 0 bad counts 0 probes changed 0 fill touched 0" % len(calls),
                                       "scan 0 bad status 0 matrix 1 subseqs 1 totals 1 fill 1", "errors -100 -100 msgs 2"], out.stdout
