"""The Python restatement of GenKMerCultsCnts / GenKMerCultThreadRange (tests/cults_ref.py) against what the reference handed to its
callback and returned (tests/golden/cults_cases.xz), field for field; kit4b_amd.kmermarkers_fasta, fed from the restatement,
against the files the reference's front end wrote (tests/golden/cults_<run>.fa.xz); and each crafted case takes the branch it
was made for.  No device."""
import io
import lzma
import os
import struct
from collections import Counter

import numpy as np
import pytest

import cults_craft as cc
import cults_ref
import query_ref

RUNS = [("cults_k20", dict(kmer_len=20)), ("cults_k24_p20_s2", dict(kmer_len=24, prefix_len=20, min_shared=2)),
        ("cults_k20_sense_s1", dict(kmer_len=20, min_shared=1, sense_only=True))]
EOS = 7  # eBaseEOS
_cache = {}


def load_cases(golden_dir):
    if "g" not in _cache:
        with lzma.open(os.path.join(golden_dir, "cults_cases.xz"), "rb") as f:
            _cache["g"] = dict(np.load(io.BytesIO(f.read())))
    return _cache["g"]


def load_index(oracle, golden_dir, tmp_path_factory):
    """(path of the unpacked .sfx, (seq, sa, entries)), once per session"""
    if "ix" not in _cache:
        p = tmp_path_factory.mktemp("cults") / "cults_index.sfx"
        with lzma.open(os.path.join(golden_dir, "cults_index.sfx.xz"), "rb") as f:
            p.write_bytes(f.read())
        h = oracle.open(str(p))
        _cache["ix"] = (str(p), query_ref.index_from_oracle(oracle, h))
        oracle.close(h)
    return _cache["ix"]


def parse_callbacks(blob, klen):
    """the recorded callbacks (make_golden_cults.py) as the restatement's records, without `head`, which the reference does not tell"""
    raw, out, o = bytes(blob), [], 0
    while o < len(raw):
        sense, anti, ncult, tot, dense_ok, nnz = struct.unpack_from("<QQIIII", raw, o)
        o += 32
        seq = raw[o:o + klen + 1]
        o += klen + 1
        cult = [struct.unpack_from("<III", raw, o + 12 * j) for j in range(nnz)]
        o += 12 * nnz
        out.append(dict(seq=seq, sense=sense, anti=anti, ncult=ncult, tot=tot, dense_ok=dense_ok, cult=cult))
    return out


def restated(index, kw, rng, callback=None):
    """(rc, records in the golden's shape) of one case"""
    rc, recs = cults_ref.gen_kmer_cults_cnts(index, kw["sense_only"], rng[0], rng[1], kw["plen"], kw["slen"], kw["min_cult"], kw["max_homo"], callback)
    return rc, [dict(seq=r["seq"] + b"\xff", sense=r["sense"], anti=r["anti"], ncult=len(r["cult"]), tot=len(index[2]), dense_ok=1, cult=r["cult"])
                for r in recs]


@pytest.fixture(scope="module")
def index(oracle, golden_dir, tmp_path_factory):
    return load_index(oracle, golden_dir, tmp_path_factory)[1]


def all_results(index, golden_dir):
    """{case name: (range or None, rc, records with head)} of the restatement, computed once and shared with test_gpu_cults.py"""
    if "res" not in _cache:
        g = load_cases(golden_dir)
        res = {}
        for i, (name, kw, rng) in enumerate(cc.cases()):
            r = (int(g["start"][i]), int(g["end"][i]))
            if r == (-1, -1):
                res[name] = (None, 0, [])
                continue
            rc, recs = cults_ref.gen_kmer_cults_cnts(index, kw["sense_only"], r[0], r[1], kw["plen"], kw["slen"], kw["min_cult"], kw["max_homo"])
            res[name] = (r, rc, recs)
        _cache["res"] = res
    return _cache["res"]


def test_the_index_is_the_crafted_one(index):
    names, ts = cc.targets()
    seq, sa, entries = index
    assert len(entries) == 5 and [e[2] for e in entries] == [len(t) for t in ts] and len(sa) == len(seq)
    for (eid, start, ln), t in zip(entries, ts):
        assert bytes(b & 0x0F for b in seq[start:start + ln]) == t.tobytes()


def test_restatement_equals_the_recorded_callbacks(index, golden_dir):
    g = load_cases(golden_dir)
    res = all_results(index, golden_dir)
    for i, (name, kw, rng) in enumerate(cc.cases()):
        r, rc, recs = res[name]
        assert rc == int(g["rc"][i]), name
        want = parse_callbacks(g["cb_%d" % i], kw["plen"] + kw["slen"])
        got = [dict(seq=x["seq"] + b"\xff", sense=x["sense"], anti=x["anti"], ncult=len(x["cult"]), tot=5, dense_ok=1, cult=x["cult"]) for x in recs]
        assert len(got) == len(want), name
        for a, b in zip(got, want):
            assert a["seq"][:-1] == b["seq"][:-1] and b["seq"][-1] == EOS and {k: v for k, v in a.items() if k != "seq"} == \
                {k: v for k, v in b.items() if k != "seq"}, (name, a, b)
    assert sum(len(res[c[0]][2]) for c in cc.cases()) > 5000


def test_thread_ranges_and_resolved_ranges(index, golden_dir):
    g = load_cases(golden_dir)
    k = 0
    for i, (name, kw, rng) in enumerate(cc.cases()):
        r = cc.resolve(rng, index, cults_ref.thread_range)
        assert (r or (-1, -1)) == (int(g["start"][i]), int(g["end"][i])), name
        if isinstance(rng, tuple) and rng[0] == "thread":
            start = 0
            for t in range(1, rng[2] + 1):
                rc, end = cults_ref.thread_range(index, cc.P, t, rng[1], start)
                if t < rng[2] and rc >= 1:
                    start = end + 1
            assert (rc, end) == (int(g["tr_rc"][k]), int(g["tr_end"][k])), name
            k += 1
    assert k == 10


def test_aborting_callback(index, golden_dir):
    g = load_cases(golden_dir)
    seen = []

    def cb(rec):
        seen.append(rec)
        return -7 if len(seen) == 3 else 0

    kw = cc.cases()[2][1]
    rc, recs = restated(index, kw, (0, 0), cb)
    assert rc == int(g["abort_rc"][0]) == -7 and len(recs) == 3
    want = parse_callbacks(g["abort_cb"], kw["plen"] + kw["slen"])
    assert [(x["seq"][:-1], x["sense"], x["anti"], x["cult"]) for x in recs] == [(x["seq"][:-1], x["sense"], x["anti"], x["cult"]) for x in want]


def test_each_crafted_site_takes_its_branch(index, golden_dir):
    seq, sa, entries = index
    n = len(seq)
    res = all_results(index, golden_dir)
    fl = cults_ref.flags(index, cc.P, cc.S, 0, n - 1)
    pre = lambda i: bytes(b & 0x0F for b in seq[sa[i]:sa[i] + cc.P])
    by_prefix = lambda name, m: [r for r in res[name][2] if r["seq"][:cc.P] == m.tobytes()]
    # shared by all five, and a subset on both sides of MinCultivars
    assert len(res["all_cultivars"][2]) > 50 and all(len(r["cult"]) == 5 for r in res["all_cultivars"][2])
    n3, n1 = len(res["min3"][2]), len(res["min1"][2])
    assert len(res["all_cultivars"][2]) < n3 < n1 and res["min5_is_all"][2] == res["all_cultivars"][2]
    assert res["min3"][1] == res["min1"][1] == res["all_cultivars"][1] == n1 > n3  # located, reported or not (with MinCultivars 1 every located K-mer is reported)
    # N inside a prefix: elements that are neither too short nor F, whose prefix holds the N
    assert any(not x and not f and 4 in pre(i) for i, (x, f, b) in enumerate(fl))
    # M1: the run's first element has N in its suffix and is no head; the last is skipped; two members are counted
    m1 = [i for i in range(n) if pre(i) == cc.M1.tobytes()]
    assert len(m1) == 4 and m1 == list(range(m1[0], m1[0] + 4)) and fl[m1[0]][2] and [fl[i][1] for i in m1] == [False, True, True, False]
    (r,) = by_prefix("min1", cc.M1)
    assert r["head"] == m1[1] and r["sense"] == 2 and [c[0] for c in r["cult"]] == [1, 2]
    # M2: cultE's last 15 bases are too short, start a run of their own in the middle of M2's, and M2 is located twice
    m2 = [i for i in range(n) if pre(i) == cc.M2.tobytes()]
    assert [fl[i][0] for i in m2] == [False, True, False] and [fl[i][2] for i in m2] == [True, True, False]
    two = by_prefix("min1", cc.M2)
    assert len(two) == 2 and [x["head"] for x in two] == [m2[0], m2[2]] and [x["sense"] for x in two] == [1, 1]
    assert len(by_prefix("no_suffix_min1", cc.M2)) == 1 and by_prefix("no_suffix_min1", cc.M2)[0]["sense"] == 3  # (S = 0: long enough)
    # the palindrome counts its own loci again
    (r,) = by_prefix("min1", cc.PAL)
    assert r["sense"] == r["anti"] == 2 and r["cult"] == [(1, 1, 1), (3, 1, 1)]
    assert by_prefix("sense_only_min1", cc.PAL)[0]["cult"] == [(1, 1, 0), (3, 1, 0)]
    # M3: cultD only antisense; cultE's antisense hit has N behind it and counts only without a suffix
    (r,) = by_prefix("min1", cc.M3)
    assert r["cult"] == [(1, 1, 0), (2, 1, 0), (4, 0, 1)]
    assert by_prefix("no_suffix_min1", cc.M3)[0]["cult"] == [(1, 1, 0), (2, 1, 0), (4, 0, 1), (5, 0, 1)]
    assert len(by_prefix("min3", cc.M3)) == 1 and len(by_prefix("sense_only_min1", cc.M3)[0]["cult"]) == 2
    # the repeat and the homopolymers: one entry many times; a run and an antisense range of more than 64 elements
    assert any(r["cult"] == [(2, 30, 0)] or (len(r["cult"]) == 1 and r["cult"][0][1] >= 29) for r in res["min1"][2])
    (a,) = by_prefix("min1", np.zeros(cc.P, np.uint8))
    (t,) = by_prefix("min1", np.full(cc.P, 3, np.uint8))
    assert a["sense"] > 64 and a["anti"] > 64 and t["sense"] > 64 and t["anti"] == a["sense"] and a["anti"] == t["sense"]
    # ranges inside the A run: one K-mer with the elements of the range alone; the antisense side still sees the whole index
    (lo, hi), (mr, rc, recs) = cc.longest_run(index), res["mid_run"][:3]
    assert lo < mr[0] < mr[1] < hi and rc == 1 and recs[0]["sense"] == mr[1] - mr[0] + 1 and recs[0]["anti"] == a["anti"] and recs[0]["head"] == mr[0]
    assert res["one_element"][1] == 1 and res["one_element"][2][0]["sense"] == 1 and res["start_eq_n"][1:] == (0, [])
    assert res["min2_end_n1"][0] == (0, n - 1) and res["tail"][0][1] > n
    assert res["p200_s100"][1] > 0 and len(res["p200_s100"][2][0]["seq"]) == 300 and res["p5_min1"][1] > 500
    assert all(res[c[0]][1] == -1 for c in cc.cases() if c[0].startswith("err_")) and res["homozygotic_unsupported"][1] == cults_ref.UNSUPPORTED
    assert res["no_suffix_homo_ignored"][1] == res["no_suffix_min1"][1]


@pytest.mark.parametrize("run,kw", RUNS)
def test_kmermarkers_fasta_equals_the_front_end(index, golden_dir, run, kw):
    import kit4b_amd

    with lzma.open(os.path.join(golden_dir, run + ".fa.xz"), "rb") as f:
        want = f.read().decode().splitlines()
    got = kit4b_amd.kmermarkers_fasta(cults_ref.RefIndex(index), **kw).splitlines()

    def records(lines):
        assert len(lines) % 2 == 0
        ids = [int(h.split()[0][len(">KMerM"):]) for h in lines[0::2]]
        assert ids == list(range(1, len(ids) + 1))
        keys = [tuple(int(v) for v in h.split()[1].split("|")) for h in lines[0::2]]
        order = [(k[2], k[3] + k[4]) for k in keys]
        assert all(order[i] >= order[i + 1] for i in range(len(order) - 1))
        return Counter(zip(keys, lines[1::2]))

    assert len(want) >= 4 and records(got) == records(want)
    plen = kw.get("prefix_len", kw["kmer_len"])
    r = cults_ref.RefIndex(index).kmer_cults(plen, kw["kmer_len"] - plen, kw.get("min_shared", 0) or 5, sense_only=kw.get("sense_only", False))
    prefixes = [b[:plen].tobytes() for b in r["bases"]]
    assert len(set(prefixes)) == len(prefixes) > 0  # no prefix is reported twice: the duplicate flag has nothing to decide


# ---- the large cultivar set: GenKMerCultThreadRange's search for a boundary, ranges that share a K-mer, several threads -----------
def load_big(golden_dir):
    if "big" not in _cache:
        with lzma.open(os.path.join(golden_dir, "cults_big.xz"), "rb") as f:
            _cache["big"] = dict(np.load(io.BytesIO(f.read())))
    return _cache["big"]


def big_index(oracle):
    """(seq, sa, entries) of cults_craft.big_targets() from the project's own builder, once per session (make_golden_cults.py checks
    that it holds the reference's text at every place of the suffix array)"""
    if "bigix" not in _cache:
        names, ts = cc.big_targets()
        h = oracle.build(names, ts, dataset="cultsbig", threads=4)
        _cache["bigix"] = query_ref.index_from_oracle(oracle, h)
        oracle.close(h)
    return _cache["bigix"]


def test_big_thread_ranges_equal_the_reference(oracle, golden_dir):
    """2, 3 and 4 threads: every thread is active, every boundary was moved off its putative place by the search (the end is the
    first element of the next K-mer), in the restatement and in the package's host function"""
    import kit4b_amd

    ix, g = big_index(oracle), load_big(golden_dir)
    seq, sa, entries = ix
    n = len(seq)
    want = [tuple(int(v) for v in row) for row in g["tr"]]
    assert [(nt,) + r for nt in cc.BIG_THREADS for r in cc.thread_ranges(ix, cults_ref.thread_range, nt)] == want
    starts = [e[1] for e in entries]

    def bases_at(psn, k):
        e = entries[max(np.searchsorted(starts, psn, side="right") - 1, 0)]
        return seq[psn:min(psn + k, e[1] + e[2])] if e[1] <= psn < e[1] + e[2] else b""

    def pkg(_, klen, t, nt, start):
        return kit4b_amd.kmer_cult_thread_range(n, lambda i: sa[i], bases_at, klen, t, nt, start)

    assert [(nt,) + r for nt in cc.BIG_THREADS for r in cc.thread_ranges(ix, pkg, nt)] == want
    assert sum(1 for r in want if r[0] == 4 and r[3] == 1) == 4
    moved = 0
    for nt, t, start, rc, end in want:
        if t < nt:
            putative = start + (n - start) // (1 + nt - t)
            assert rc == 1 and end > putative and sa[end] + cc.P < n
            moved += end > putative + 1
            # the end starts the next K-mer: its prefix differs from the putative element's, and the elements between share that one's
            pre = lambda i: seq[sa[i]:sa[i] + cc.P]
            assert pre(end) != pre(putative) and all(pre(i) == pre(putative) for i in range(putative, end))
    assert moved >= 3


def test_big_boundary_windows_and_the_kmer_both_ranges_locate(oracle, golden_dir):
    """150 elements on either side of each boundary of three threads: the restatement equals the recorded callbacks; the K-mer that
    starts at a range's inclusive end is located by that range and, with its other elements, by the next"""
    ix, g = big_index(oracle), load_big(golden_dir)
    three = [tuple(int(v) for v in r) for r in g["tr"] if r[0] == 3]
    shared = 0
    for k, (_, t, start, rc, end) in enumerate(three[:2]):
        got = []
        for j, (a, b) in enumerate(((end - 150, end), (end + 1, end + 150))):
            n, recs = cults_ref.gen_kmer_cults_cnts(ix, False, a, b, cc.P, cc.S, 1)
            want = parse_callbacks(g["win_%d" % (2 * k + j)], cc.P + cc.S)
            assert n == int(g["win_rc"][2 * k + j]) and len(recs) == len(want)
            assert [(x["seq"], x["sense"], x["anti"], x["cult"]) for x in recs] == [(x["seq"][:-1], x["sense"], x["anti"], x["cult"]) for x in want]
            got.append(recs)
        if got[0][-1]["head"] == end and got[1][0]["seq"][:cc.P] == got[0][-1]["seq"][:cc.P]:
            shared += 1
            assert got[0][-1]["sense"] == 1 and got[1][0]["head"] == end + 1
    assert shared == 2


def test_big_kmermarkers_fasta_with_four_threads(oracle, golden_dir):
    import kit4b_amd

    with lzma.open(os.path.join(golden_dir, "cults_big_k20_T4.fa.xz"), "rb") as f:
        want = f.read().decode()
    got = kit4b_amd.kmermarkers_fasta(cults_ref.RefIndex(big_index(oracle)), 20, threads=4)
    assert fasta_records(got.splitlines()) == fasta_records(want.splitlines()) and want.count(">") > 50


def fasta_records(lines):
    """a marker file as the multiset of (fields behind the id, sequence); the ids count up from 1 and the (cultivars, counts) key never rises"""
    assert len(lines) % 2 == 0
    ids = [int(h.split()[0][len(">KMerM"):]) for h in lines[0::2]]
    assert ids == list(range(1, len(ids) + 1))
    keys = [tuple(int(v) for v in h.split()[1].split("|")) for h in lines[0::2]]
    order = [(k[2], k[3] + k[4]) for k in keys]
    assert all(order[i] >= order[i + 1] for i in range(len(order) - 1))
    return Counter(zip(keys, lines[1::2]))
