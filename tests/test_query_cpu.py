"""tests/query_ref.py, the sequential Python restatement of CSfxArray::LocateQuerySeqs, against what the reference itself returned
for the crafted queries (tests/golden/query_*.xz, written by tests/golden/make_golden_query.py): every node, every field, in order.
Also: the fixtures are the crafted inputs of tests/query_craft.py, and the ABI declares the new entry points."""
import io
import lzma
import os

import numpy as np
import pytest

import query_craft as qc
import query_ref

GROUPS = ("corewalk", "extension", "redundancy", "depth", "caps")


def load_group(golden_dir, group):
    with lzma.open(os.path.join(golden_dir, "query_%s.xz" % group), "rb") as f:
        return dict(np.load(io.BytesIO(f.read())))


@pytest.fixture(scope="module")
def index(oracle, golden_dir, tmp_path_factory):
    p = tmp_path_factory.mktemp("query") / "query_index.sfx"
    with lzma.open(os.path.join(golden_dir, "query_index.sfx.xz"), "rb") as f:
        p.write_bytes(f.read())
    h = oracle.open(str(p))
    yield query_ref.index_from_oracle(oracle, h)
    oracle.close(h)


@pytest.mark.parametrize("group", GROUPS)
def test_restatement_reproduces_the_reference(index, golden_dir, group):
    g = load_group(golden_dir, group)
    cases = qc.groups()[group]
    assert [c[0] for c in cases] == list(g["names"])
    for i, (name, query, params) in enumerate(cases):
        assert np.array_equal(g["cat"][int(g["offs"][i]):int(g["offs"][i]) + int(g["lens"][i])], query), name
        assert tuple(g["params"][i]) == tuple(params), name
        want = [tuple(int(v) for v in r) for r in g["nodes"][int(g["node_offs"][i]):int(g["node_offs"][i + 1])]]
        got = query_ref.locate_query_seqs(index, query, *params)
        assert got == want, (group, name)


def test_fixtures_hold_the_cases_they_are_meant_to(golden_dir):
    """the reference's answers show the shapes the cases were crafted for"""
    def nodes(group, name):
        g = load_group(golden_dir, group)
        i = list(g["names"]).index(name)
        return g["nodes"][int(g["node_offs"][i]):int(g["node_offs"][i + 1])]

    assert len(nodes("corewalk", "len20")) == 0 and len(nodes("corewalk", "len21")) == 1
    assert len(nodes("corewalk", "final_offset_only")) == 0 and len(nodes("corewalk", "last_probed_offset")) == 1
    e = nodes("extension", "exact400")
    assert len(e) == 1 and tuple(e[0]) == (0, 400, 1, 1000, 0, 0, 0)
    assert [len(nodes("depth", "planted%d_iter5" % n)) > 0 for n in qc.DEPTH_COUNTS] == [True, False, False]
    assert all(len(nodes("depth", "planted%d_iter0" % n)) == 0 for n in qc.DEPTH_COUNTS)
    assert [len(nodes("caps", "max_hits%d" % m)) for m in (1, 2, 3)] == [1, 2, 3]
    assert any(int(r[5]) != k for k, r in enumerate(nodes("redundancy", "swallowed")))  # an earlier node was flagged and compacted away


def test_header_declares_the_query_entry_points():
    import kit4b_amd

    for s in ("k4_query_reserve", "k4_locate_query_seqs_batch", "k4_locate_query_seqs_batch_dev", "k4_query_last_kernel_ms"):
        assert s in kit4b_amd.ABI_SYMBOLS
        assert hasattr(kit4b_amd.lib(), s), s
    assert kit4b_amd.QUERY_NODE_DTYPE.itemsize == 28
