"""kalign's priority regions (`-B <bed>`, `-V`; k4align: --priorityregionfile / --nofiltpriority) on the device: k4align writes what
`ngskit4b kalign` wrote (tests/golden/make_golden_priority.py), also as BAM and under -b; the library's priority pass and
k4_filter_priority_regions_dev equal the restatement (tests/priority_ref.py); with the table cleared the library computes what it did
before a table was set."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import priority_ref
import samutil
from oracle_bindings import HIT_DTYPE, RESULT_DTYPE, Oracle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PKG = os.path.join(os.path.dirname(HERE), "kit4b_amd")
K4ALIGN = os.path.join(PKG, "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "priority_cases.json")))
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}


def _unxz(tmp_path, name):
    dst = str(tmp_path / name[:-3])
    if not os.path.exists(dst):
        open(dst, "wb").write(lzma.open(os.path.join(GOLDEN, name)).read())
    return dst


def _command(tmp_path, case, out, extra=()):
    meta = CASES[case]
    cmd = [K4ALIGN, "-I", _unxz(tmp_path, "priority.sfx.xz"), "-o", out]
    for a in meta["args"]:
        cmd.append("--nofiltpriority" if a == "-V" and case.startswith("b") else a)  # both spellings of the flag
    if meta["bed"]:
        cmd += ["--priorityregionfile", os.path.join(GOLDEN, "priority_%s.bed" % meta["bed"])]
    for flag, r in zip(("-i", "-u"), meta["reads"]):
        cmd += [flag, _unxz(tmp_path, "priority_%s.fa.xz" % r)]
    return cmd + list(extra)


def _body(path):
    return [l for l in open(path).read().split("\n") if l and not l.startswith("@")]


def _header(path):
    return [l for l in open(path).read().split("\n") if l.startswith("@") and not l.startswith("@PG")]


@pytest.mark.parametrize("case", sorted(CASES))
def test_k4align_writes_the_reference_sam(tmp_path, case):
    meta = CASES[case]
    out = str(tmp_path / "o.sam")
    p = subprocess.run(_command(tmp_path, case, out), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    for name, n in meta["nar"].items():
        assert ("%d (%s)" % (n, name)) in p.stderr, (name, n, p.stderr)
    if meta["bed"] and "-V" not in meta["args"]:
        assert ("%d matches removed by priority region filtering" % meta["nar"].get("PR", 0)) in p.stderr
    want = _unxz(tmp_path, "priority_%s.sam.xz" % case)
    got, wbody = _body(out), _body(want)
    assert _header(out) == _header(want)
    n_acc = meta["nar"]["AA"]
    assert len(got) == len(wbody) and got[:n_acc] == wbody[:n_acc]  # the alignments: line for line
    if "-M1" in meta["args"]:  # the unaligned tail: the same NAR groups in the same order, each group as a set
        code = lambda l: samutil.NAR_CODES.index(l.rsplit("YU:Z:", 1)[1])  # noqa: E731
        assert [code(l) for l in got[n_acc:]] == [code(l) for l in wbody[n_acc:]]
        assert sorted(got[n_acc:]) == sorted(wbody[n_acc:])


def test_bam_output_holds_the_reference_alignments(tmp_path):
    out = str(tmp_path / "o.bam")
    p = subprocess.run(_command(tmp_path, "a_M0", out), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    _, refs, recs = samutil.read_bam(out)
    want = [samutil.sam_line_fields(l) for l in _body(_unxz(tmp_path, "priority_a_M0.sam.xz"))]
    assert [samutil.bam_record_as_sam_fields(r, refs) for r in recs] == want and len(want) == CASES["a_M0"]["nar"]["AA"]


def test_streamed_batches_give_the_same_alignments(tmp_path):
    out = str(tmp_path / "b.sam")
    p = subprocess.run(_command(tmp_path, "a_M0", out, ["-b", "0.01"]), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    got, want = _body(out), _body(_unxz(tmp_path, "priority_a_M0.sam.xz"))
    key = lambda l: tuple(l.split("\t")[2:4])  # noqa: E731
    assert sorted(got) == sorted(want) and [key(l) for l in got] == [key(l) for l in want]
    assert p.stderr.count("matches removed by priority region filtering") > 1  # more than one batch went through the stage


# ---- the library against the restatement --------------------------------------------------------------------------------------------
def _reads(name):
    seqs = [l.strip() for l in lzma.open(os.path.join(GOLDEN, name), "rt") if not l.startswith(">")]
    return [np.array([CODE[c] for c in s], np.uint8) for s in seqs]


@pytest.fixture(scope="module")
def index(tmp_path_factory):
    import kit4b_amd

    tmp = tmp_path_factory.mktemp("priority")
    sfx = _unxz(tmp, "priority.sfx.xz")
    ix = kit4b_amd.SfxIndex.open(sfx)
    ix.set_max_iter(5000)
    # what the library computes before a table is ever set on this index: one SE and one PE golden input
    before = dict(se=ix.kalign_batch(_reads("priority_dup.fa.xz"), max_subs=2, max_ml=3, pe_mode=2),
                  pe=ix.kalign_pe_batch(_reads("priority_pe_1.fa.xz"), _reads("priority_pe_2.fa.xz"), **PE_KW))
    O = Oracle()
    h = O.open(sfx)
    O.set_max_iter(h, 5000)
    names = [e["name"] for e in O.entries(h)]
    yield ix, O, h, names, before
    ix.close()
    O.close(h)


def _regions(bed_text, names):
    return priority_ref.Regions(bed_text, names)


PE_KW = dict(pe_mode=1, pair_min_len=150, pair_max_len=600, max_subs=2)
ALL = "asm1 0 20000\ntrusted1 0 5000\ntrusted2 0 5000\nrep 0 40000\nasm2 0 5000\ntrusted3 0 5000\nuniq 0 9000\n"


@pytest.mark.parametrize("max_ml,pe_mode", [(1, 0), (3, 1), (12, 2)])
@pytest.mark.parametrize("bed", ["trusted", "two_of_three", "rep", "ALL", "FAR"])
def test_priority_pass_equals_the_restatement(index, bed, max_ml, pe_mode):
    """reads with 0, 1, 2, 3, 12 hits (unique, D, T, M copies) at hit limits 1, 3 and 12, i.e. with max_ml + 10 below and above the
    copy counts; 651 reads (no multiple of 64); ALL: every hit is a priority hit; FAR: a table no read meets, so every read takes the
    normal call"""
    ix, O, h, names, _ = index
    reads = _reads("priority_dup.fa.xz") + _reads("priority_tri.fa.xz")[:171] + _reads("priority_rep.fa.xz")[:160]
    assert len(reads) % 64 != 0
    text = ALL if bed == "ALL" else "trusted1 0 3\n" if bed == "FAR" else open(os.path.join(GOLDEN, "priority_%s.bed" % bed)).read()
    regions = _regions(text, names)
    kw = dict(max_subs=2, max_ml=max_ml, pe_mode=pe_mode)
    norm = O.kalign_batch(h, reads, **kw)
    wide = O.kalign_batch(h, reads, **dict(kw, max_ml=max_ml + priority_ref.PRIORITY_EXACTS))
    want_out, want_hits, need = priority_ref.select(regions, wide["out"], wide["hits"], norm["out"], norm["hits"], max_ml, pe_mode)
    if bed == "FAR":
        assert need.all()
    if bed == "ALL" and max_ml == 12:
        assert need.sum() == (wide["out"]["hit_rslt"] != 1).sum()
    ix.set_priority_regions(*regions.intervals())
    try:
        got = ix.kalign_batch(reads, **kw)
    finally:
        ix.set_priority_regions()
    assert np.array_equal(got["out"], want_out)
    for i in range(len(reads)):
        k = min(int(want_out[i]["inst"]), max_ml) if want_out[i]["hit_rslt"] in (1, 2, 3) else 0
        assert np.array_equal(got["hits"][i, :k], want_hits[i, :k]), i
        assert not got["hits"][i, k:].view(np.uint8).any(), i
    cleared = ix.kalign_batch(reads, **kw)
    assert np.array_equal(cleared["out"], norm["out"])


def test_filter_stage_equals_the_restatement(index):
    import torch

    ix, O, h, names, _ = index
    rng = np.random.default_rng(5)
    n = 100003  # no multiple of 64 or 256
    ents = O.entries(h)
    regions = _regions("asm1 100 200\nasm1 150 400\nasm1 400 401\nuniq 3000 3100\nrep 0 27600\nnosuch 1 2\n", names)
    out = np.zeros(n, RESULT_DTYPE)
    hits = np.zeros((n, 2), HIT_DTYPE)
    out["nar"] = rng.choice([1, 1, 1, 3, 5, 12, 9], n)
    out["num_hits"] = (out["nar"] == 1).astype(np.int32)
    out["inst"] = rng.integers(0, 4, n)
    c = rng.integers(0, len(ents) + 2, n)  # entry ids 0 and n_entries + 1 as well: no such sequence
    hits["chrom_id"][:, 0] = c
    hits["match_loci"][:, 0] = np.where(rng.random(n) < 0.5, rng.integers(0, 600, n), rng.integers(2800, 3300, n))
    hits["match_len"][:, 0] = rng.integers(1, 151, n)
    hits["strand"][:, 0] = rng.choice([43, 45], n)
    hits[:, 1] = hits[:, 0]
    nar, num_hits, hits0 = out["nar"].copy(), out["num_hits"].copy(), hits[:, 0].copy()
    want = priority_ref.filter_regions(regions, nar, num_hits, hits0)
    assert 0 < want < (out["nar"] == 1).sum()
    d_rr = torch.from_numpy(out.view(np.uint8).reshape(n, -1).copy()).cuda()
    d_hits = torch.from_numpy(hits.view(np.uint8).reshape(n, -1).copy()).cuda()
    ix.set_priority_regions(*regions.intervals())
    try:
        got = ix.filter_priority_regions(n, 2, d_rr=d_rr, d_hits=d_hits)
        again = ix.filter_priority_regions(n, 2, d_rr=d_rr, d_hits=d_hits)
    finally:
        ix.set_priority_regions()
    assert got == want and again == 0
    g_out = d_rr.cpu().numpy().view(RESULT_DTYPE).reshape(n)
    g_hits = d_hits.cpu().numpy().view(HIT_DTYPE).reshape(n, 2)
    assert np.array_equal(g_out["nar"], nar) and np.array_equal(g_out["num_hits"], num_hits) and np.array_equal(g_out["inst"], out["inst"])
    assert np.array_equal(g_hits[:, 0], hits0) and np.array_equal(g_hits[:, 1], hits[:, 1])


def test_a_cleared_table_gives_what_the_library_gave_before_any_table(index):
    ix, O, h, names, before = index
    r1, r2 = _reads("priority_pe_1.fa.xz"), _reads("priority_pe_2.fa.xz")
    dup = _reads("priority_dup.fa.xz")
    regions = _regions(open(os.path.join(GOLDEN, "priority_trusted.bed")).read(), names)
    ix.set_priority_regions(*regions.intervals())
    with_pe = ix.kalign_pe_batch(r1, r2, **PE_KW)
    with_se = ix.kalign_batch(dup, max_subs=2, max_ml=3, pe_mode=2)
    ix.set_priority_regions()
    after_pe = ix.kalign_pe_batch(r1, r2, **PE_KW)
    after_se = ix.kalign_batch(dup, max_subs=2, max_ml=3, pe_mode=2)
    assert np.array_equal(before["pe"], after_pe) and not np.array_equal(before["pe"], with_pe)
    assert np.array_equal(before["se"]["out"], after_se["out"]) and np.array_equal(before["se"]["hits"], after_se["hits"])
    assert not np.array_equal(before["se"]["out"], with_se["out"])


@pytest.mark.parametrize("shape", ["mixed", "none_needs_normal", "all_need_normal"])
@pytest.mark.parametrize("max_ml,pe_mode", [(1, 0), (3, 1), (5, 2)])
def test_select_kernel_equals_the_restatement_on_synthetic_records(index, shape, max_ml, pe_mode):
    """k4_priority_select_dev on 100 003 synthetic wide records (no multiple of 64 or 256): reads with 0, 1, max_ml, max_ml + 1,
    exactly max_ml + 10 and more instances (inst beyond the slots: the walk stops at max_ml + 10), results other than eHRhits, hits
    on sequence ids 0 and n_entries + 1, priority hits in front of, between and behind outsiders; a batch in which no read needs the
    normal pass and one in which all do"""
    import torch

    ix, O, h, names, _ = index
    rng = np.random.default_rng(17 + max_ml)
    n, wide = 100003, max_ml + priority_ref.PRIORITY_EXACTS
    ents = O.entries(h)
    bed = "asm1 1000 3000\nasm1 2500 4000\nuniq 3000 3100\nuniq 5000 5000\nrep 0 27600\ntrusted1 100 200\n"
    if shape == "none_needs_normal":  # every sequence covered whole
        bed = "".join("%s 0 %d\n" % (e["name"], e["seq_len"] + 200) for e in ents)
    if shape == "all_need_normal":
        bed = "uniq 7000 7100\n"  # behind every locus the hits are drawn from
    regions = _regions(bed, names)
    w_out = np.zeros(n, RESULT_DTYPE)
    w_hits = np.zeros((n, wide), HIT_DTYPE)
    inst = rng.choice([0, 1, 1, 2, max_ml, max_ml + 1, wide - 1, wide, wide + 1, wide + 7], n).astype(np.int32)
    w_out["inst"] = inst
    w_out["hit_rslt"] = np.where(inst == 0, 0, rng.choice([1, 1, 1, 1, 2, 3], n))
    w_out["low_mm"], w_out["nxt_mm"] = rng.integers(0, 3, n), rng.integers(3, 6, n)
    if shape == "none_needs_normal":  # 1..max_ml instances, all eHRhits, all on real sequences
        w_out["inst"] = inst = rng.integers(1, max_ml + 1, n).astype(np.int32)
        w_out["hit_rslt"] = 1
        w_hits["chrom_id"] = rng.integers(1, len(ents) + 1, (n, wide))
        w_hits["match_loci"] = rng.integers(0, 400, (n, wide))
    else:
        w_hits["chrom_id"] = rng.integers(0, len(ents) + 2, (n, wide))
        w_hits["match_loci"] = np.where(rng.random((n, wide)) < 0.5, rng.integers(0, 6000, (n, wide)), rng.integers(2850, 3150, (n, wide)))
    w_hits["match_len"] = rng.integers(1, 151, (n, wide))
    w_hits["strand"] = rng.choice([43, 45], (n, wide))
    w_hits["mismatches"] = rng.integers(0, 3, (n, wide))
    w_hits["reserved"] = rng.integers(0, 1 << 28, (n, wide))
    n_out = np.zeros(n, RESULT_DTYPE)
    n_out["nar"] = 77  # what the caller's records held: a read that needs the normal pass keeps it
    n_hits = np.zeros((n, max_ml), HIT_DTYPE)
    want_out, want_hits, need = priority_ref.select(regions, w_out, w_hits, n_out, n_hits, max_ml, pe_mode)
    if shape == "none_needs_normal":
        assert not need.any()
    elif shape == "all_need_normal":
        assert need.all()
    else:
        assert 0.1 * n < need.sum() < 0.9 * n
        k = want_out["inst"][~need]
        assert set(range(1, max_ml + 1)) <= set(k.tolist())  # exactly max_ml priority hits among them
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(len(a), -1).copy()).cuda()  # noqa: E731
    d_wout, d_whits, d_out, d_hits = dev(w_out), dev(w_hits), dev(n_out), dev(n_hits)
    d_need = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    ix.set_priority_regions(*regions.intervals())
    try:
        ix.priority_select(n, max_ml, d_wout, d_whits, d_out, d_hits, d_need, pe_mode=pe_mode)
        torch.cuda.synchronize()
    finally:
        ix.set_priority_regions()
    g_need = d_need.cpu().numpy()
    g_out = d_out.cpu().numpy().view(RESULT_DTYPE).reshape(n)
    g_hits = d_hits.cpu().numpy().view(HIT_DTYPE).reshape(n, max_ml)
    assert np.array_equal(g_need, need.astype(np.uint8))
    assert np.array_equal(g_out, want_out)
    assert np.array_equal(g_hits[~need], want_hits[~need])
