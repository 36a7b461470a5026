"""The Python restatement of LocateAllNearMatches and of genzygosity's scan (tests/zyg_ref.py) against what the reference returned
(tests/golden/zygosity_calls.xz), field for field; kit4b_amd.genzygosity_csv, fed from the restatement, against the files the
reference's front end wrote (tests/golden/zygosity_<case>[_raw].csv.xz), byte for byte; an entry shorter than -l; the new symbols
are declared.  No device."""
import io
import lzma
import os
import re

import numpy as np
import pytest

import query_ref
import zyg_craft as zc
import zyg_ref as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ("max_tot_mm", "core_len", "core_delta", "max_core_slides", "max_matches", "num_entries", "probe_entry", "probe_ofs")
_cache = {}


def load_calls(golden_dir):
    if "g" not in _cache:
        with lzma.open(os.path.join(golden_dir, "zygosity_calls.xz"), "rb") as f:
            _cache["g"] = dict(np.load(io.BytesIO(f.read())))
    return _cache["g"]


def load_index(oracle, golden_dir, tmp_path_factory):
    """(path of the unpacked .sfx, (seq, sa, entries)), once per session"""
    if "ix" not in _cache:
        p = tmp_path_factory.mktemp("zygosity") / "zygosity_index.sfx"
        with lzma.open(os.path.join(golden_dir, "zygosity_index.sfx.xz"), "rb") as f:
            p.write_bytes(f.read())
        h = oracle.open(str(p))
        _cache["ix"] = (str(p), query_ref.index_from_oracle(oracle, h))
        oracle.close(h)
    return _cache["ix"]


def call_list(g):
    """the recorded calls as dicts: the columns, the probe, and the reference's rslt and counts"""
    out = []
    for i in range(len(g["lens"])):
        c = {k: int(g[k][i]) for k in COLS + ("cur_max_iter", "n_ident_nodes", "rslt")}
        c["probe"] = g["cat"][int(g["offs"][i]):int(g["offs"][i]) + int(g["lens"][i])]
        c["cnt"] = g["cnt"][int(g["cnt_offs"][i]):int(g["cnt_offs"][i + 1])].tolist()
        out.append(c)
    return out


def scan_kw(kw):
    return {k: v for k, v in kw.items() if k != "threshold"}


def scan_results(index):
    """{file stem: (matrix, subseqs, totals, status)} of the restatement, computed once and shared with test_gpu_zygosity.py"""
    if "scan" not in _cache:
        _cache["scan"] = {stem: zr.zygosity(index, **scan_kw(kw)) for stem, kw in zc.scan_cases()}
    return _cache["scan"]


def golden_file(golden_dir, name):
    with lzma.open(os.path.join(golden_dir, name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def index(oracle, golden_dir, tmp_path_factory):
    return load_index(oracle, golden_dir, tmp_path_factory)[1]


def test_the_index_is_the_crafted_one(index):
    names, seqs, sites = zc.build()
    seq, sa, entries = index
    assert 6 <= len(entries) <= 8 and [e[2] for e in entries] == [len(t) for t in seqs] and len(sa) == len(seq)
    assert [e[0] for e in entries] == list(range(1, len(entries) + 1)) and all(2000 <= len(t) <= 6000 for t in seqs)
    for (eid, start, ln), t in zip(entries, seqs):
        assert bytes(b & 0x0F for b in seq[start:start + ln]) == t.tobytes()
    runs = zr._runs(index, 11)
    assert runs[bytes([0, 1] * 5 + [0])][1] > 1100 and 1000 < runs[bytes([0, 2] * 5 + [0])][1] < 1098


def test_restatement_equals_the_recorded_returns(index, golden_dir):
    g = load_calls(golden_dir)
    calls = call_list(g)
    want = zc.calls(*zc.build()[1:])
    assert len(calls) >= 400 and [c["probe"].tolist() for c in calls] == [c["probe"].tolist() for c in want]
    stats, ordered = {}, 0
    for i, c in enumerate(calls):
        s = {}
        r, cnt = zr.near_matches(index, *[c[k] for k in COLS], c["probe"].tobytes(), c["cur_max_iter"], c["n_ident_nodes"], s)
        assert (r, cnt) == (c["rslt"], c["cnt"]), i
        for k in s:
            stats[k] = stats.get(k, 0) + 1  # calls, not walks
        ordered += zr.needs_ordered_walk(index, c["probe"].tobytes(), c["core_len"], c["core_delta"], c["max_core_slides"], c["cur_max_iter"], c["n_ident_nodes"])
    assert stats["own_entry"] >= 20 and stats["too_many"] >= 20 and stats["truncated"] >= 20 and stats["node_cut"] >= 5, stats
    assert 20 <= ordered < len(calls) - 100
    for k, vals in (("max_matches", (0, 1, 3)), ("cur_max_iter", (0, 50, 1000)), ("n_ident_nodes", (3, 40, 1024000)), ("max_core_slides", (1, 3, 8))):
        assert set(vals) <= set(c[k] for c in calls), k
    assert min(c["num_entries"] for c in calls) < len(index[2]) and max(c["rslt"] for c in calls) > 3


def test_core_offsets_and_limits_of_the_front_end():
    import kit4b_amd

    for args in ((30000, 25, 2, 0), (30000, 25, 2, 3), (3 * 10 ** 8, 50, 4, 2), (21000000, 20, 0, 1), (30000, 1000, 30, 2)):
        assert kit4b_amd.genzygosity_limits(*args) == zr.derive(*args), args
    assert zr.core_offsets(25, 9, 9, 4) == [0, 9, 16] and zr.core_offsets(25, 11, 11, 3) == [0, 11]
    assert zr.core_offsets(50, 10, 10, 8) == [0, 10, 20, 30, 40] and zr.core_offsets(20, 20, 20, 4) == [0]
    assert zr.derive(30000, 25, 2, 0) == (9, 4, 5000) and zr.derive(30000, 25, 2, 3) == (11, 3, 1000) and zr.derive(3 * 10 ** 8, 50, 4, 2) == (10, 8, 50000)


@pytest.mark.parametrize("stem,kw", zc.scan_cases())
def test_genzygosity_csv_equals_the_front_end(index, golden_dir, stem, kw):
    import kit4b_amd

    m, s, tot, status = scan_results(index)[stem]
    ref = zr.RefIndex(index, zc.NAMES)
    ref.zygosity = lambda **k: (m, s, tot)  # (the scan computed once)
    thr, raw = kit4b_amd.genzygosity_csv(ref, **kw)
    assert thr == golden_file(golden_dir, stem + ".csv.xz") and raw == golden_file(golden_dir, stem + "_raw.csv.xz")
    assert len(raw.splitlines()) == 64 and 0 < len(thr.splitlines()) < 64
    assert tot["windows"] == tot["passed_over"] + tot["rejected"] + tot["unique"] and tot["passed_over"] > 0 and tot["rejected"] > 0
    assert int(s.sum()) == tot["unique"] and len(status) == sum(e[2] for e in index[2]) and set(np.unique(status)) == {0, 1, 2, 3}


def test_the_m3_run_takes_the_ordered_walk(index):
    res = scan_results(index)
    assert res["zygosity_l25_s2_m3_x3"][2]["ordered"] > 1000 and res["zygosity_l25_s2"][2]["ordered"] == 0


def test_an_entry_shorter_than_the_window_has_a_zero_row(oracle, tmp_path):
    names, seqs = zc.short_entry()
    h = oracle.build(names, seqs, dataset="zygshort", threads=2)
    ix = query_ref.index_from_oracle(oracle, h)
    oracle.close(h)
    m, s, tot, status = zr.zygosity(ix, 25, 2)
    assert not m[1].any() and s[1] == 0 and not m[:, 1].any() and m[0, 2] > 0 and m[2, 0] > 0  # no source windows; none fits into it either
    assert len(status) == sum(len(t) for t in seqs) and tot["windows"] == sum(max(0, len(t) - 24) for t in seqs)


def test_parameter_errors_of_the_restatement(index):
    for kw in zc.error_cases():
        assert zr.check_params(index, **kw) == zr.ERR_PARAMS, kw
    assert zr.check_params(index) == 0 and zr.check_params(index, src_first=8, src_count=1) == 0


def test_new_symbols_are_declared_and_bound():
    import kit4b_amd

    header = open(os.path.join(ROOT, "include", "k4sfx.h")).read()
    names = ["k4_all_near_matches_batch", "k4_all_near_matches_batch_dev", "k4_zygosity_batch", "k4_zygosity_batch_dev", "k4_zygosity_last_kernel_ms"]
    src = open(os.path.join(ROOT, "kit4b_amd", "csrc", "k4_zygosity.hip")).read()
    for n in names:
        assert re.search(r"\b%s\(" % n, header) and re.search(r'extern "C" \w+ %s\(' % n, src), n
    for n in ("k4_near_params", "k4_zygosity_params", "k4_zygosity_totals"):
        assert n in header, n
    assert "k4_zygosity.hip" in open(os.path.join(ROOT, "kit4b_amd", "csrc", "Makefile")).read()
    for n in ("genzygosity_csv", "genzygosity_limits", "NearParams", "ZygosityParams", "ZygosityTotals"):
        assert hasattr(kit4b_amd, n), n
    for n in ("all_near_matches", "zygosity", "zygosity_kernel_ms"):
        assert hasattr(kit4b_amd.SfxIndex, n), n
    facade = open(os.path.join(ROOT, "include", "k4_sfxarray.hpp")).read()
    for n in ("LocateAllNearMatches", "ZygosityBatch"):
        assert n in facade, n
