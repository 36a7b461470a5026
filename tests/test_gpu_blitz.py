"""CBlitz's path stage on the device (k4_blitz.hip) through the C ABI and the Python binding: record for record against the Python
restatement (tests/blitz_ref.py, pinned to the reference by test_blitz_cpu.py) and line for line against the PSL lines the
reference itself wrote (tests/golden/blitz_*.xz)."""
import ctypes as C
import lzma
import os

import numpy as np
import pytest

import blitz_craft as bc
import blitz_ref
import manytargets as mt
import query_craft as qc
import query_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


@pytest.fixture(scope="module")
def sfx_path(golden_dir, tmp_path_factory):
    p = tmp_path_factory.mktemp("blitz") / "query_index.sfx"
    with lzma.open(os.path.join(golden_dir, "query_index.sfx.xz"), "rb") as f:
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


def _lkw(lp):
    return dict(zip(qc.PARAM_NAMES, (int(v) for v in lp)))


def _pkw(pp):
    return dict(zip(blitz_ref.PARAM_NAMES, (int(v) for v in pp)))


def _restated(ref, qs, lp, pp):
    """(paths with the batch's query index and block_off, blocks) of the restatement over a batch"""
    paths, blocks = [], []
    for i, q in enumerate(qs):
        nodes = query_ref.locate_query_seqs(ref, q, *lp)
        ps, bs = blitz_ref.blitz_paths(ref, q, nodes, *pp, query_idx=i)
        paths += [p[:16] + (p[16] + len(blocks),) for p in ps]
        blocks += bs
    return paths, blocks


def _rows(a, fields):
    return [tuple(int(r[f]) for f in fields) for r in a]


def _check(got, want):
    path_offs, paths, blocks = got
    assert _rows(paths, blitz_ref.PATH_FIELDS) == want[0]
    assert _rows(blocks, blitz_ref.BLOCK_FIELDS) == want[1]
    per_query = np.bincount([p[0] for p in want[0]], minlength=len(path_offs) - 1) if want[0] else np.zeros(len(path_offs) - 1, int)
    assert [int(v) for v in np.diff(path_offs.astype(np.int64))] == [int(v) for v in per_query]


@pytest.mark.parametrize("group", bc.GROUPS)
def test_golden_cases_record_for_record_and_line_for_line(k4, ix, ref_index, golden_dir, group):
    """every crafted case through k4_blitz_paths_batch against the restatement, and through both device stages (SfxIndex.blitz, the
    _dev entries) and psl_lines against what the reference wrote; the host-pointer and the _dev entries agree"""
    lp, pp, cases = bc.groups()[group]
    qs = [c[1] for c in cases]
    nodes = ix.locate_query_seqs(qs, **_lkw(lp))
    host = ix.blitz_paths(qs, None, nodes, **_pkw(pp))
    _check(host, _restated(ref_index, qs, lp, pp))
    kw = _lkw(lp)
    kw.update(_pkw(pp))
    dev = ix.blitz(qs, **kw)
    for a, b in zip(host, dev):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert k4.psl_lines(ix, [c[0] for c in cases], qs, dev[1], dev[2]) == bc.golden_lines(golden_dir, group)
    assert ix.blitz_ms[0] > 0 and (ix.blitz_ms[1] > 0 or len(dev[1]) == 0)


@pytest.mark.parametrize("pp", (bc._path(max_paths=2, query_len_aligned_pct=50), bc._path(min_path_score=10, query_len_aligned_pct=10, max_paths=3),
                                bc._path(max_paths=2, query_len_aligned_pct=50, strand=2)))
def test_mixed_batch_with_empty_slots(ix, ref_index, pp):
    """0 to 5000 bases in one batch; queries without a node at the start, in the middle and at the end, and queries whose nodes make
    no path; a configured minimum under 25 is floored"""
    qs, lp, _ = bc.mixed_batch()
    nodes = ix.locate_query_seqs(qs, **_lkw(lp))
    n_nodes = [len(a) for a in nodes]
    assert n_nodes[0] == 0 and n_nodes[-1] == 0 and 0 in n_nodes[2:-1]
    got = ix.blitz_paths(qs, None, nodes, **_pkw(pp))
    want = _restated(ref_index, qs, lp, pp)
    _check(got, want)
    per_query = np.diff(got[0].astype(np.int64))
    assert per_query[0] == 0 and per_query[-1] == 0 and len(want[0]) > 0
    if pp[6] == 0 and pp[3] == 0:
        assert any(per_query[i] == 0 and n_nodes[i] > 0 for i in range(len(qs)))  # nodes, but no path


def test_blocks_trimmed_to_zero_length_are_unlinked(k4, ix, ref_index):
    """hand-made nodes (blitz_craft.unlinked) whose overlap trims consume a whole node, as the current and as the next one, on both
    strands: the kernel's two unlink branches against the restatement's, which has to reach both"""
    cases, pp, want = bc.unlinked()
    qs = [c[1] for c in cases]
    counters, paths, blocks = {}, [], []
    for i, (_, q, nodes) in enumerate(cases):
        ps, bs = blitz_ref.blitz_paths(ref_index, q, nodes, *pp, query_idx=i, counters=counters)
        paths += [p[:16] + (p[16] + len(blocks),) for p in ps]
        blocks += bs
    assert counters.get("zero_len_cur", 0) > 0 and counters.get("zero_len_next", 0) > 0 and len(paths) == len(cases)
    per_query = [query_ref.as_array(c[2], k4.QUERY_NODE_DTYPE) for c in cases]
    _check(ix.blitz_paths(qs, None, per_query, **_pkw(pp)), (paths, blocks))


def test_nodes_on_a_query_under_8_bases_are_ignored(k4, ix, ref_index):
    """no node fits such a query; hand-made ones on a query of 4 and of 0 bases give no path (and no division by the length), the
    query behind them in the batch still gets its own"""
    cases, pp, _ = bc.unlinked()
    stray = [(0, 8, 1, 100, 0, 0, 0), (0, 8, 1, 200, 0, 0, 1)]
    qs = [np.zeros(4, np.uint8), np.zeros(0, np.uint8), cases[0][1]]
    per_query = [query_ref.as_array(n, k4.QUERY_NODE_DTYPE) for n in (stray, stray, cases[0][2])]
    pp = pp[:3] + (0,) + pp[4:]  # the automatic minimum: (length - 5) * match / 3
    want = blitz_ref.blitz_paths(ref_index, qs[2], cases[0][2], *pp, query_idx=2)
    assert len(want[0]) == 1 and blitz_ref.blitz_paths(ref_index, qs[0], stray, *pp) == ([], [])
    got = ix.blitz_paths(qs, None, per_query, **_pkw(pp))
    _check(got, want)
    assert [int(v) for v in got[0]] == [0, 0, 0, 1]


@pytest.fixture(scope="module")
def built(k4, oracle):
    made = []

    def make(names, chroms, el):
        h = oracle.build(names, chroms, dataset="q", force_el=el if el == 5 else 0, threads=4)
        cat = oracle.concat_len(h)
        sa_raw = np.ctypeslib.as_array(C.cast(oracle.L.k4o_sa_bytes(h), C.POINTER(C.c_uint8)), shape=(cat * el,))
        x = k4.SfxIndex.from_host(np.array(oracle.seq(h)), sa_raw, el, k4.make_entries(names, [len(c) for c in chroms]), dataset="q")
        made.append((x, h))
        return x, query_ref.index_from_oracle(oracle, h)

    yield make
    for x, h in made:
        x.close()
        oracle.close(h)


def test_260_targets(built):
    """the entry table is searched in global memory above 128 targets: paths on targets 4, 132 and 260, both strands"""
    names, chroms = mt.small_genome(260)
    x, ref = built(names, chroms, 4)
    a, b, c = chroms[3], chroms[131], chroms[259]
    q = np.concatenate([a[:110], b[5:60], b[75:115], qc.revcomp(a[10:118]), c[:100], b[:60]])
    lp = qc._p(core_len=12, core_delta=3, max_hits=200000, match_pts=1, mismatch_pts=2)
    pp = bc._path(query_len_aligned_pct=5, min_path_score=25, max_paths=4)
    qs = [q, qc.revcomp(q)]
    got = x.blitz_paths(qs, None, x.locate_query_seqs(qs, **_lkw(lp)), **_pkw(pp))
    want = _restated(ref, qs, lp, pp)
    _check(got, want)
    assert {p[1] for p in want[0]} >= {4, 132, 260} and {p[2] for p in want[0]} == {0, 1}


def test_five_byte_suffix_elements(k4, built, golden_dir):
    names, ts = qc.targets()
    x, _ = built(names, ts, 5)
    assert x.info()["sfx_el_size"] == 5
    lp, pp, cases = bc.groups()["default"]
    kw = _lkw(lp)
    kw.update(_pkw(pp))
    qs = [c[1] for c in cases]
    _, paths, blocks = x.blitz(qs, **kw)
    assert k4.psl_lines(x, [c[0] for c in cases], qs, paths, blocks) == bc.golden_lines(golden_dir, "default")


def test_capacity_protocol_and_argument_errors(k4, ix):
    """a paths or blocks capacity one short returns K4_ERR_MEM with the sizes needed and leaves every output untouched"""
    lp, pp, cases = bc.groups()["default"]
    qs = [np.ascontiguousarray(c[1]) for c in cases]
    per_query = ix.locate_query_seqs(qs, **_lkw(lp))
    _, want_paths, want_blocks = ix.blitz_paths(qs, None, per_query, **_pkw(pp))
    n_p, n_b = len(want_paths), len(want_blocks)
    assert n_p > 2 and n_b > n_p
    cat, offs, lens = k4._flatten(qs)
    node_offs = np.concatenate([[0], np.cumsum([len(a) for a in per_query])]).astype(np.uint64)
    nodes = np.concatenate(per_query)
    L, n = k4.lib(), len(qs)
    p = k4.BlitzParams(*pp)

    def call(paths_cap, blocks_cap, params=p):
        path_offs = np.full(n + 1, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        paths = np.full((n_p + 2) * 72, 0xEE, dtype=np.uint8).view(k4.BLITZ_PATH_DTYPE)
        blocks = np.full((n_b + 2) * 12, 0xEE, dtype=np.uint8).view(k4.BLITZ_BLOCK_DTYPE)
        needed = np.zeros(2, dtype=np.uint64)
        rc = L.k4_blitz_paths_batch(ix.h, C.byref(params), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data, node_offs.ctypes.data,
                                    nodes.ctypes.data, path_offs.ctypes.data, paths.ctypes.data, paths_cap, blocks.ctypes.data, blocks_cap,
                                    needed.ctypes.data)
        return rc, path_offs, paths, blocks, [int(v) for v in needed]

    for caps in ((n_p - 1, n_b), (n_p, n_b - 1)):
        rc, path_offs, paths, blocks, needed = call(*caps)
        assert rc == -95 and needed == [n_p, n_b] and b"paths_cap" in L.k4_last_error(ix.h)
        assert all((a.view(np.uint8) == 0xEE).all() for a in (path_offs, paths, blocks))
    rc, path_offs, paths, blocks, needed = call(n_p, n_b)
    assert rc == 0 and needed == [n_p, n_b] and int(path_offs[n]) == n_p
    assert paths[:n_p].tobytes() == want_paths.tobytes() and blocks[:n_b].tobytes() == want_blocks.tobytes()
    assert (paths[n_p:].view(np.uint8) == 0xEE).all() and (blocks[n_b:].view(np.uint8) == 0xEE).all()
    with pytest.raises(k4.K4Error) as e:
        ix.blitz_paths(qs, None, per_query, paths_cap=1, **_pkw(pp))
    assert e.value.code == -95 and e.value.needed == (n_p, n_b)
    for bad in (dict(match_pts=0), dict(mismatch_pts=11), dict(gap_open=0), dict(min_path_score=-1), dict(query_len_aligned_pct=0),
                dict(query_len_aligned_pct=101), dict(max_paths=0), dict(max_paths=11), dict(strand=3)):
        rc = call(n_p, n_b, k4.BlitzParams(*bc._path(**bad)))[0]
        assert rc == -100 and list(bad)[0].encode() in L.k4_last_error(ix.h), bad
