"""tests/blitz_ref.py, the sequential Python restatement of CBlitz's path stage, against the PSL lines `ngskit4b blitz` itself wrote
for the crafted queries (tests/golden/blitz_*.xz, written by tests/golden/make_golden_blitz.py): every line, every column, in order.
Also: every case reaches the branch it was crafted for, HighScoreSW's fill order never meets an unscored successor (blitz_ref
asserts it for every successor; here: that successors were met at all), and the ABI declares the new entry points.

Not reached by a golden: a block trimmed to zero length and unlinked (with 20-base cores two trims of at most 8 bases cannot
consume a node), and a configured minimum score under 25 (`-p` refuses it; the floor is exercised through the automatic minimum
only for queries under 80 bases, which the reference filters out).  The restatement and the kernel carry both branches.  For the
first, blitz_craft.unlinked() makes nodes by hand: here the restatement has to reach both unlink branches on them and is checked
against what ConsolidateNodes (:2157-2320) leaves, worked out by hand; test_gpu_blitz.py compares the device with it on the
same nodes, and on a minimum of 10 for the second."""
import lzma
import os

import pytest

import blitz_craft as bc
import blitz_ref
import query_ref

GROUPS = bc.GROUPS
golden_lines = bc.golden_lines


@pytest.fixture(scope="module")
def index(oracle, golden_dir, tmp_path_factory):
    p = tmp_path_factory.mktemp("blitz") / "query_index.sfx"
    with lzma.open(os.path.join(golden_dir, "query_index.sfx.xz"), "rb") as f:
        p.write_bytes(f.read())
    h = oracle.open(str(p))
    ents = {e["entry_id"]: (e["name"], e["seq_len"]) for e in oracle.entries(h)}
    yield query_ref.index_from_oracle(oracle, h), ents
    oracle.close(h)


def restated(index, ents, cases, lp, pp, counters):
    lines = []
    for name, q in cases:
        nodes = query_ref.locate_query_seqs(index, q, *lp)
        paths, blocks = blitz_ref.blitz_paths(index, q, nodes, *pp, counters=counters)
        for p in paths:
            tid, nb, off = p[1], p[15], p[16]
            lines.append(blitz_ref.psl_line(name, len(q), ents[tid][0], ents[tid][1], p, blocks[off:off + nb]))
    return lines


@pytest.mark.parametrize("group", GROUPS)
def test_restatement_reproduces_the_reference_lines(index, golden_dir, group):
    ix, ents = index
    lp, pp, cases = bc.groups()[group]
    counters = {}
    assert restated(ix, ents, cases, lp, pp, counters) == golden_lines(golden_dir, group)
    for k in bc.WANT[group]:
        assert counters.get(k, 0) > 0, (group, k)
    if group in ("default", "groups", "paths3"):
        assert counters["successors"] > 0  # (each one passed the fill-order assertion of blitz_ref._score_group)


def test_restatement_unlinks_a_block_trimmed_to_zero_length(index):
    """hand-made nodes (blitz_craft.unlinked): the unlink branches of ConsolidateNodes fire, each on the side it was crafted for, and
    leave the blocks a reading of :2250-2303 gives: the consumed node is gone; consumed as the current node it has taken over its
    successor's length and link, but kept its own, trimmed, start"""
    ix, _ = index
    cases, pp, want = bc.unlinked()
    assert set(want.values()) == {"zero_len_cur", "zero_len_next"}
    for name, q, nodes in cases:
        counters = {}
        paths, blocks = blitz_ref.blitz_paths(ix, q, nodes, *pp, counters=counters)
        assert counters.get(want[name], 0) == 1 and counters.get("overlap_trimmed", 0) > 0, (name, counters)
        a, m, b = (nd[3] for nd in nodes)
        kept = (40, 40, b) if want[name] == "zero_len_next" else (40, 40, m + 8)
        assert blocks == [(40, 0, a), kept], name
        assert len(paths) == 1 and paths[0][2] == nodes[0][6] and paths[0][15] == 2, name


def test_fixtures_hold_the_cases_they_are_meant_to(golden_dir):
    d = {ln.split("\t")[9]: ln.split("\t") for ln in golden_lines(golden_dir, "default")}
    assert d["exact400"][17:] == ["1", "400,", "0,", "1000,"] and d["exact400"][:8] == ["400"] + ["0"] * 7
    assert d["del30"][4:8] == ["0", "0", "1", "30"] and d["ins30"][4:8] == ["1", "30", "0", "0"] and d["ins30_del30"][17] == "3"
    assert d["merge20"][17] == "1" and d["merge20"][1] == "20"           # two nodes and the 20 bases between them, merged
    assert d["del30_rc"][8] == "-" and d["n_in_block"][3] == "1" and "overlap9" not in d
    assert d["close2"][18] == "151,151," and d["close7"][18] == "154,153,"    # the closed gaps went to both sides
    assert len(golden_lines(golden_dir, "paths1")) == 2 and len(golden_lines(golden_dir, "paths3")) == 6
    assert [ln.split("\t")[9] for ln in golden_lines(golden_dir, "pct_cut")] == ["lesser_alone"]
    assert {ln.split("\t")[8] for ln in golden_lines(golden_dir, "paths3_minus")} == {"-"}


def test_header_declares_the_blitz_entry_points():
    import kit4b_amd

    for s in ("k4_blitz_paths_batch", "k4_blitz_paths_batch_dev", "k4_blitz_last_kernel_ms"):
        assert s in kit4b_amd.ABI_SYMBOLS
        assert hasattr(kit4b_amd.lib(), s), s
    assert kit4b_amd.BLITZ_PATH_DTYPE.itemsize == 72 and kit4b_amd.BLITZ_BLOCK_DTYPE.itemsize == 12
