"""tests/hamm_ref.py, the sequential Python restatement of CSfxArray::LocateSfxHammings / LocateHammings / LocateHamming, against
what the reference itself returned for the crafted spans (tests/golden/hamm_cases.xz, written by tests/golden/make_golden_hamm.py),
byte for byte; kit4b_amd.hammings_csv / hamming_spans against what `ngskit4b hammings -m0` wrote and logged over the same index;
and each crafted case takes the branch it was made for."""
import io
import json
import lzma
import os

import numpy as np
import pytest

import hamm_craft as hc
import hamm_ref
import kit4b_amd
import query_ref


def load_cases(golden_dir):
    with lzma.open(os.path.join(golden_dir, "hamm_cases.xz"), "rb") as f:
        return dict(np.load(io.BytesIO(f.read())))


def load_run(golden_dir, run):
    with lzma.open(os.path.join(golden_dir, run + ".xz"), "rb") as f:
        return np.frombuffer(f.read(), dtype=np.uint8)


def distribution(entry_lens, hammings, kmer_len, rhamm):
    """the tally GenRestrictedHammings logs (ngskit4b/hammings.cpp:2535-2587): bytes under 0x7f over the K-mer loci of every entry,
    and once more the byte behind the last entry's last K-mer"""
    hist, sampled, unsampled, base, k = [0] * 256, 0, 0, 0, 0
    for ln in entry_lens:
        k = base
        base += ln
        if ln < kmer_len:
            continue
        for k in range(base - ln, base - kmer_len + 1):
            if hammings[k] < 0x7F:
                sampled += 1
                hist[int(hammings[k])] += 1
            else:
                unsampled += 1
        k += 1
    if hammings[k] < 0x7F:
        sampled += 1
        hist[int(hammings[k])] += 1
    else:
        unsampled += 1
    return dict(sampled=sampled, unsampled=unsampled, counts=hist[:rhamm + 1] + [hist[rhamm + 1]])


@pytest.fixture(scope="module")
def index(oracle, golden_dir, tmp_path_factory):
    p = tmp_path_factory.mktemp("hamm") / "hamm_index.sfx"
    with lzma.open(os.path.join(golden_dir, "hamm_index.sfx.xz"), "rb") as f:
        p.write_bytes(f.read())
    h = oracle.open(str(p))
    yield query_ref.index_from_oracle(oracle, h)
    oracle.close(h)


def run_ref(index, case, stats=None):
    name, form, what, p, _ = case
    rhamm, both, nth, mn, mx, iib = p
    n = what[2] if form == "sfx" else len(what)
    out = np.full(n, 0xFF, dtype=np.uint8)
    if form == "sfx":
        rc = hamm_ref.locate_sfx_hammings(index, rhamm, bool(both), hc.K, nth, what[2], mn, mx, what[0], what[1], iib, out, stats=stats)
    else:
        rc = hamm_ref.locate_hammings(index, rhamm, bool(both), hc.K, nth, what, mn, mx, iib, out, stats=stats)
    return rc, out


@pytest.fixture(scope="module")
def restated(index):
    """every crafted case through the restatement, once: {name: (rc, bytes, stats)}"""
    res = {}
    for c in hc.cases():
        st = {}
        rc, out = run_ref(index, c, st)
        res[c[0]] = (rc, out, st)
    return res


def test_index_is_the_crafted_targets(index):
    names, ts = hc.targets()
    seq, _, entries = index
    assert [e[2] for e in entries] == [len(t) for t in ts]
    for e, t in zip(entries, ts):
        assert np.array_equal(np.frombuffer(seq[e[1]:e[1] + e[2]], dtype=np.uint8) & 0x0F, t)


def test_restatement_reproduces_the_reference(restated, golden_dir):
    g = load_cases(golden_dir)
    cases = hc.cases()
    assert [c[0] for c in cases] == list(g["names"])
    for i, c in enumerate(cases):
        rc, out, _ = restated[c[0]]
        assert rc == int(g["rc"][i]) == 0, c[0]
        assert np.array_equal(out, g["out_%d" % i]), (c[0], out[:16], g["out_%d" % i][:16])
        if c[4]:
            for ofs, v in c[4].items():
                assert int(g["out_%d" % i][ofs]) == v, (c[0], ofs)


def _stats(restated, name):
    """the counters of the case's only K-mer: one dict per N substitution"""
    st = restated[name][2]["kmers"]
    assert len(st) == 1
    return next(iter(st.values()))


def test_each_case_takes_the_branch_it_was_made_for(restated):
    s = lambda name: _stats(restated, name)  # noqa: E731
    for r in range(1, 7):  # a unique K-mer runs every stage up to rhamm and none finds anything
        st = s("unique_r%d" % r)[0]
        assert st["last_stage"] == (0, 2, 3, 4, 5, 5)[r - 1] and "found" not in st
    for d in range(1, 7):  # the neighbour at distance d is found by the stage (d, d) -- (0, 1) for d = 1, (5, 6) for 5 and 6
        st = s("near%d" % d)[0]
        assert st["found"][0] == (0, 2, 3, 4, 5, 5)[d - 1] and st["found"][3] == d and st["last_stage"] == st["found"][0]
        if d > 1:
            assert "found" not in s("near%d_r%d" % (d, d - 1))[0]
    assert s("copy_intra_z0")[0].get("self_skip") == 1 and "filter_skip" not in s("copy_intra_z0")[0]
    assert s("copy_inter_z1")[0].get("filter_skip", 0) >= 1 and s("copy_intra_z2")[0].get("filter_skip", 0) >= 1
    assert s("near1_z1")[0]["found"][3] == 1 and s("intra_near_z2")[0]["found"][3] == 1
    assert s("palindrome_both")[0].get("self_skip") == 1 and s("palindrome_both")[0]["last_stage"] == 0
    assert s("rev_only_both")[0]["last_stage"] == 0 and "found" not in s("rev_only_both")[0]  # the exact antisense pass
    assert s("dup_segment")[0].get("dup_skip", 0) >= 1
    assert s("eos_cross")[0].get("eos_break", 0) >= 1
    assert s("before_start")[0].get("before_start", 0) >= 1
    assert s("past_end")[0].get("past_end", 0) >= 1
    assert len(s("n1")) == 4 and len(s("n2")) == 16 and len(s("n4")) == 256  # every substitution is tried: none reaches 0
    assert 1 <= len(s("n1_closer")) <= 4 and s("n1_closer")[-1]["last_stage"] == 0
    assert restated["n5"][2].get("kmers") is None  # more than 4 N: no search at all
    assert s("n_in_neighbour")[0]["found"][3] == 1
    assert s("depth_inside")[0].get("capped") == 1 and "abandoned" not in s("depth_inside")[0] and "found" in s("depth_inside")[0]
    assert s("depth_beyond")[0].get("capped") == 1 and "found" not in s("depth_beyond")[0]
    assert "capped" not in s("depth_all")[0] and "found" in s("depth_all")[0]
    assert s("depth_abandoned")[0].get("abandoned") == 1 and "found" not in s("depth_abandoned")[0]
    assert s("depth_abandoned_early")[0].get("abandoned") == 1 and "found" in s("depth_abandoned_early")[0]


def test_sampled_span_leaves_the_other_bytes(restated):
    out = restated["span_nth3"][1]
    assert (out[np.arange(len(out)) % 3 != 0] == 0xFF).all() and (out[0:len(out) - hc.K + 1:3] != 0xFF).all()
    assert (out[len(out) - hc.K + 1:] == 0xFF).all()


def test_parameter_errors_of_the_reference(index):
    out = np.full(100, 0xFF, dtype=np.uint8)
    for kw in (dict(entry_id=0), dict(span_len=hc.K - 1), dict(entry_loci=3000 - hc.K + 1), dict(entry_id=9), dict(rhamm=0), dict(kmer_len=9, span_len=9)):
        a = dict(rhamm=3, kmer_len=hc.K, span_len=hc.K, entry_id=1, entry_loci=0)
        a.update(kw)
        assert hamm_ref.locate_sfx_hammings(index, a["rhamm"], False, a["kmer_len"], 1, a["span_len"], 3, 4, a["entry_id"], a["entry_loci"], 0,
                                            out) == hamm_ref.ERR_INTERNAL, kw
    assert (out == 0xFF).all()


@pytest.mark.parametrize("run,kw", hc.CSV_RUNS)
def test_report_and_span_cut_reproduce_the_front_end(golden_dir, run, kw):
    """hammings_csv over the bytes the engine calls left equals the front end's file byte for byte; for the sampled run, which
    writes no file, the logged distribution pins the span cut (h4 is longer than the 10 000-base MaxHammSeqLen: its second span
    starts at 9941, which is no multiple of 3)"""
    names, ts = hc.targets()
    lens = [len(t) for t in ts]
    arr = load_run(golden_dir, run)
    assert len(arr) == sum(lens)
    nth = kw.get("sample_nth", 1)
    ids, locis, sl, offs = kit4b_amd.hamming_spans(lens, kw["kmer_len"])
    written = np.zeros(len(arr), dtype=bool)
    for lo, n, o in zip(locis, sl, offs):
        written[int(o):int(o) + int(n) - kw["kmer_len"] + 1:nth] = True
    assert ((arr != 0xFF) == written).all()
    assert list(ids) == [1, 2, 3, 4, 4] and int(locis[4]) == 10000 - kw["kmer_len"] + 1
    if nth == 1:
        with lzma.open(os.path.join(golden_dir, run + ".csv.xz"), "rb") as f:
            want = f.read().decode()
        assert kit4b_amd.hammings_csv(names, lens, arr, kw["kmer_len"]) == want
    else:
        want = json.load(open(os.path.join(golden_dir, run + ".dist.json")))
        assert distribution(lens, arr, kw["kmer_len"], kw["rhamm"]) == want


def test_report_run_loop_quirks():
    """byte 0 is compared with itself first and the loop's locus runs one ahead of the byte it reads, so a run that does not start
    at 0 is reported one base late; the byte of the last K-mer is never read"""
    h = np.array([3, 3, 1, 1, 1, 2, 9, 0xFF, 0xFF], dtype=np.uint8)  # 9 bases, K = 3: K-mers at 0..6
    assert kit4b_amd.hammings_csv(["c"], [9], h, 3) == '"Chrom","StartLoci","Len","Hamming"\n"c",0,2,3\n"c",3,3,1\n"c",6,1,2\n'
    assert kit4b_amd.hammings_csv(["a", "b"], [2, 3], np.array([0xFF, 0xFF, 7, 0xFF, 0xFF], dtype=np.uint8), 3).endswith('\n"b",0,0,7\n')


def test_header_declares_the_hamming_entry_points():
    import ctypes as C

    for s in ("k4_locate_sfx_hammings_batch", "k4_locate_sfx_hammings_batch_dev", "k4_locate_hammings_batch", "k4_locate_hammings_batch_dev",
              "k4_hamming_last_kernel_ms"):
        assert s in kit4b_amd.ABI_SYMBOLS
        assert hasattr(kit4b_amd.lib(), s), s
    assert C.sizeof(kit4b_amd.HammingParams) == 28
