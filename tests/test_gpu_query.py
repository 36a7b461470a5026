"""LocateQuerySeqs on the device (k4_query.hip) through the C ABI, the Python binding and the C++ facade: the reference's own
answers (tests/golden/query_*.xz) and, on fresh inputs, the Python restatement that test_query_cpu.py pins to them.  Every node
is compared field by field, in order."""
import ctypes as C
import lzma
import os
import subprocess

import numpy as np
import pytest

import manytargets as mt
import query_craft as qc
import query_ref
from test_query_cpu import GROUPS, load_group

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


@pytest.fixture(scope="module")
def sfx_path(golden_dir, tmp_path_factory):
    p = tmp_path_factory.mktemp("query") / "query_index.sfx"
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


def _params(p):
    return dict(zip(qc.PARAM_NAMES, (int(v) for v in p)))


def _rows(a):
    return [tuple(int(r[f]) for f in query_ref.NODE_FIELDS) for r in a]


def _golden_rows(g, i):
    return [tuple(int(v) for v in r) for r in g["nodes"][int(g["node_offs"][i]):int(g["node_offs"][i + 1])]]


def _by_params(cases):
    by = {}
    for i, c in enumerate(cases):
        by.setdefault(tuple(c[2]), []).append(i)
    return by


@pytest.mark.parametrize("group", GROUPS)
def test_binding_returns_the_reference_nodes(ix, golden_dir, group):
    """core walk, extension, containment / redundancy, depth, caps and wave edges: one batch per parameter set"""
    g = load_group(golden_dir, group)
    cases = qc.groups()[group]
    for p, idx in _by_params(cases).items():
        got = ix.locate_query_seqs([cases[i][1] for i in idx], **_params(p))
        for k, i in enumerate(idx):
            assert got[k].dtype == ix_dtype() and _rows(got[k]) == _golden_rows(g, i), (group, cases[i][0])


def ix_dtype():
    import kit4b_amd

    return kit4b_amd.QUERY_NODE_DTYPE


def test_c_abi_batch_and_nodes_cap(k4, ix, golden_dir):
    """k4_locate_query_seqs_batch itself: compact output behind node_offs; a capacity one short returns K4_ERR_MEM, the needed total
    in node_offs[n] and leaves nodes untouched; argument errors carry a message"""
    g = load_group(golden_dir, "caps")
    cases = qc.groups()["caps"]
    idx = _by_params(cases)[qc._p(core_delta=1)]
    qs = [np.ascontiguousarray(cases[i][1]) for i in idx]
    cat, offs, lens = k4._flatten(qs)
    want = [r for i in idx for r in _golden_rows(g, i)]
    L, n = k4.lib(), len(qs)
    p = k4.QueryParams(*qc._p(core_delta=1))
    node_offs = np.zeros(n + 1, dtype=np.uint64)
    nodes = np.full(len(want) + 4, 0xEE, dtype=np.uint8).repeat(28).view(k4.QUERY_NODE_DTYPE)
    args = (ix.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data, node_offs.ctypes.data, nodes.ctypes.data)
    assert L.k4_locate_query_seqs_batch(*args, len(want) - 1) == -95
    assert int(node_offs[n]) == len(want) and b"nodes_cap" in L.k4_last_error(ix.h)
    assert (nodes.view(np.uint8) == 0xEE).all()
    assert L.k4_locate_query_seqs_batch(*args, len(want)) == 0
    assert _rows(nodes[:len(want)]) == want and (nodes[len(want):].view(np.uint8) == 0xEE).all()
    assert [int(v) for v in np.diff(node_offs)] == [int(g["node_offs"][i + 1] - g["node_offs"][i]) for i in idx]
    with pytest.raises(k4.K4Error) as e:
        ix.locate_query_seqs(qs, nodes_cap=3, **_params(qc._p(core_delta=1)))
    assert e.value.needed == len(want)
    for bad in (dict(core_len=7), dict(core_len=101), dict(core_delta=0), dict(max_hits=0)):
        pb = k4.QueryParams(*qc._p(**bad))
        assert L.k4_locate_query_seqs_batch(ix.h, C.byref(pb), n, *args[3:], len(want)) == -100
        assert list(bad)[0].encode() in L.k4_last_error(ix.h)


@pytest.mark.parametrize("strand", (0, 1, 2))
def test_mixed_batch_equals_each_query_alone_and_the_restatement(ix, ref_index, strand):
    """lengths 0, 20, 21 .. 20 000 in one batch"""
    qs, p = qc.batch()
    kw = _params(p)
    kw["strand"] = strand
    got = ix.locate_query_seqs(qs, **kw)
    assert len(got[0]) == 0 and len(got[2]) == 0
    for q, a in zip(qs, got):
        assert _rows(a) == _rows(ix.locate_query_seqs([q], **kw)[0])
        assert _rows(a) == query_ref.locate_query_seqs(ref_index, q, *[kw[k] for k in qc.PARAM_NAMES]), len(q)
    assert sum(len(a) for a in got) > (0 if strand == 2 else 5)  # (one query of the batch is a reverse complement, the others are not)


def test_batches_without_a_core_give_all_zero_offsets(k4, ix):
    """a batch of no queries, and one whose queries are all no longer than core_len: node_offs comes back all zero and no node is
    written; then a batch one query shorter than the one before it, whose total is read where that one kept a count"""
    L = k4.lib()
    p = k4.QueryParams(*qc._p())
    core_len = dict(zip(qc.PARAM_NAMES, qc._p()))["core_len"]
    rng = np.random.default_rng(11)
    for qs in ([], [rng.integers(0, 4, m).astype(np.uint8) for m in (0, 1, core_len - 1, core_len, core_len)]):
        cat, offs, lens = k4._flatten(qs)
        cat = np.concatenate([cat, np.zeros(16, np.uint8)])
        n = len(qs)
        node_offs = np.full(n + 1, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        nodes = np.full(8 * 28, 0xEE, dtype=np.uint8).view(k4.QUERY_NODE_DTYPE)
        assert L.k4_locate_query_seqs_batch(ix.h, C.byref(p), n, cat.ctypes.data, offs.ctypes.data, lens.ctypes.data, node_offs.ctypes.data,
                                            nodes.ctypes.data, len(nodes)) == 0
        assert not node_offs.any() and (nodes.view(np.uint8) == 0xEE).all(), n
        got = ix.locate_query_seqs(qs, **_params(qc._p()))
        assert len(got) == n and all(len(a) == 0 for a in got)
    qs, pq = qc.batch()
    full = ix.locate_query_seqs(qs, **_params(pq))
    assert len(full[len(qs) - 2]) > 0  # (its count sits where the shorter batch's scan ends)
    part = ix.locate_query_seqs(qs[:-1], **_params(pq))
    assert [_rows(a) for a in part] == [_rows(a) for a in full[:-1]]


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


def test_targets_whose_ids_differ_by_128_share_a_chain(built):
    """260 targets (the entry table is searched in global memory): one query made of pieces of targets 4, 132 and 260 -- ids 4 and
    132 hash alike -- on both strands"""
    names, chroms = mt.small_genome(260)
    x, ref = built(names, chroms, 4)
    a, b, c = chroms[3], chroms[131], chroms[259]
    q = np.concatenate([a[:110], b[5:115], qc.revcomp(a[10:118]), c[:100], b[:60]])
    for kw in (dict(core_len=12, core_delta=3), dict(core_len=20, core_delta=10, max_hits=2)):
        p = qc._p(**kw)
        got = [_rows(r) for r in x.locate_query_seqs([q, qc.revcomp(q)], **_params(p))]
        assert got == [query_ref.locate_query_seqs(ref, v, *p) for v in (q, qc.revcomp(q))]
        assert {r[2] for r in got[0]} >= ({4, 132} if "max_hits" not in kw else set())


def test_five_byte_suffix_elements(built, golden_dir):
    """the crafted targets indexed with 5-byte elements: the extension group as the reference answered it"""
    names, ts = qc.targets()
    x, _ = built(names, ts, 5)
    assert x.info()["sfx_el_size"] == 5
    g = load_group(golden_dir, "extension")
    cases = qc.groups()["extension"]
    for p, idx in _by_params(cases).items():
        got = x.locate_query_seqs([cases[i][1] for i in idx], **_params(p))
        for k, i in enumerate(idx):
            assert _rows(got[k]) == _golden_rows(g, i), cases[i][0]


def test_csfxarray_query_facade_program(sfx_path, golden_dir, tmp_path):
    """eight threads call CSfxArray::LocateQuerySeqs of include/k4_sfxarray.hpp at once: each gets the fixture's nodes in the
    reference's tsQueryAlignNodes layout; InitOverOccKMers(20, 4) gives a call with a huge CurMaxIter the depth 5"""
    exe = os.path.join(ROOT, "kit4b_amd", "k4_query_facade_test")
    assert os.path.exists(exe), "make -C kit4b_amd/csrc"
    lines, n_q, n_nodes = [], 0, 0
    for group in ("depth", "redundancy", "extension", "caps"):
        g = load_group(golden_dir, group)
        for i, (name, q, p) in enumerate(qc.groups()[group]):
            rows = _golden_rows(g, i)
            lines.append(" ".join(str(v) for v in (len(q),) + tuple(p) + (len(rows),)))
            lines.append("".join(str(int(b)) for b in q) or "-")
            lines += [" ".join(str(v) for v in r) for r in rows]
            n_q, n_nodes = n_q + 1, n_nodes + len(rows)
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, sfx_path, str(cases), "4"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    o = out.stdout.splitlines()
    assert o[0] == "threads 8 queries %d nodes %d bad 0 msgs 0" % (n_q, n_nodes), out.stdout
    depth = load_group(golden_dir, "depth")
    by_name = {c[0]: int(depth["node_offs"][i + 1] - depth["node_offs"][i]) for i, c in enumerate(qc.groups()["depth"])}
    want = [by_name["planted%d_iter5" % n] for n in qc.DEPTH_COUNTS for _ in range(3)]  # whatever the case's own max_iter
    assert [int(v) for v in o[1].split(":")[1].split()[:9]] == want, o[1]
    assert o[2] == "core_len 7 -> -100 msgs 1", o[2]
