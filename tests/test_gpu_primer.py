"""kalign's 5' PCR primer correction (`-6 <n>`) on the device: k4align writes what `ngskit4b kalign` / `genpba` wrote
(tests/golden/make_golden_primer.py) -- also through -b, -S i/N + k4merge and -G --, and k4_pcr5_primer_correct_dev leaves, byte for
byte, what the literal restatement (tests/primer_ref.py) leaves on 100 000 crafted records over g1 (tests/primer_craft.py)."""
import json
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

import primer_craft
import samutil
import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PKG = os.path.join(os.path.dirname(HERE), "kit4b_amd")
K4ALIGN, K4MERGE = os.path.join(PKG, "k4align"), os.path.join(PKG, "k4merge")
CASES = json.load(open(os.path.join(GOLDEN, "primer_cases.json")))
MARKS = json.load(lzma.open(os.path.join(GOLDEN, "primer_marks.json.xz"), "rt"))
TOTALS = "PCR 5' primer correction: %d reads with %d bases corrected, %d reads with excessive substitutions rejected"


def _unxz(tmp_path, name):
    dst = str(tmp_path / name[:-3])
    if not os.path.exists(dst):
        open(dst, "wb").write(lzma.open(os.path.join(GOLDEN, name)).read())
    return dst


def _golden(case, kind):
    return lzma.open(os.path.join(GOLDEN, "primer_%s.%s.xz" % (case, kind))).read()


def _command(tmp_path, case, out, extra=()):
    meta = CASES[case]
    sfx = os.path.join(GOLDEN, "g1.sfx") if meta["index"] == "g1" else _unxz(tmp_path, "g3.sfx.xz")
    cmd = [K4ALIGN, "-I", sfx, "-o", out]
    for a in meta["args"]:
        cmd += [a, out + (".stats.csv" if a == "-O" else ".none.fa")] if a in ("-O", "-j") else [a]
    if meta["out"] == "pba":
        cmd += ["-M3", "--experimentid", meta["ids"][0], "--readsetid", meta["ids"][1]]
    for flag, r in zip(("-i", "-u"), meta["reads"]):
        cmd += [flag, _unxz(tmp_path, r)]
    return cmd + list(extra)


def _body(path):
    return [l for l in open(path).read().split("\n") if l and not l.startswith("@")]


def _same_alignments(got, want):
    """the same lines in the same coordinate order; lines of one position may come in another order (batches, slices: ties fall in
    batch order there, the reference leaves them open)"""
    key = lambda l: tuple(l.split("\t")[2:4])  # noqa: E731
    return sorted(got) == sorted(want) and [key(l) for l in got] == [key(l) for l in want]


def _header(path):
    return [l for l in open(path).read().split("\n") if l.startswith("@") and not l.startswith("@PG")]


@pytest.mark.parametrize("case", sorted(CASES))
def test_k4align_writes_the_reference_output(tmp_path, case):
    meta = CASES[case]
    out = str(tmp_path / ("o." + meta["out"]))
    p = subprocess.run(_command(tmp_path, case, out), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert (TOTALS % tuple(meta["totals"])) in p.stderr, p.stderr
    if meta["out"] == "pba":  # genpba reports through its two files
        assert open(out, "rb").read() == _golden(case, "pba")
        assert open(str(tmp_path / "o.covsegs.wig"), "rb").read() == _golden(case, "covsegs.wig")
        return
    for name, n in meta["nar"].items():
        assert ("%d (%s)" % (n, name)) in p.stderr, (name, n)
    if meta["out"] == "bam":
        text, refs, recs = samutil.read_bam(out)
        wtext, wrefs, wrecs = samutil.read_bam(os.path.join(GOLDEN, "primer_%s.bam" % case))
        assert refs == wrefs
        assert [l for l in text.splitlines() if not l.startswith("@PG")] == [l for l in wtext.splitlines() if not l.startswith("@PG")]
        key = lambda r: (r["ref"], r["pos"], r["name"], r["flag"])  # noqa: E731
        assert sorted(recs, key=key) == sorted(wrecs, key=key) and len(recs) == meta["nar"]["AA"]
        return
    want = _unxz(tmp_path, "primer_%s.sam.xz" % case)
    got, wbody = _body(out), _body(want)
    assert _header(out) == _header(want)
    n_acc = sum(1 for l in wbody if "YU:Z:" not in l)
    assert len(got) == len(wbody) and got[:n_acc] == wbody[:n_acc]  # the alignments: line for line, corrected SEQ included
    if "-M1" in meta["args"]:  # the unaligned tail: the same NAR groups in the same order, each group as a set
        code = lambda l: samutil.NAR_CODES.index(l.rsplit("YU:Z:", 1)[1])  # noqa: E731
        assert [code(l) for l in got[n_acc:]] == [code(l) for l in wbody[n_acc:]]
        assert sorted(got[n_acc:]) == sorted(wbody[n_acc:])
        assert sorted(l.split("\t", 2)[0] + "/" + str((int(l.split("\t", 2)[1]) >> 7) & 1) for l in got if l.endswith("YU:Z:NL")) == MARKS[case]
    if "-p5" in meta["args"]:
        assert open(out + ".snp", "rb").read() == _golden(case, "snp")
    if "-j" in meta["args"]:
        assert open(out + ".none.fa", "rb").read() == _golden(case, "none")
    for kind, path in (("main", out + ".stats.csv"), ("cnts", out + ".stats.AlignCntsDist.csv")):
        if kind in meta["files"]:
            assert open(path, "rb").read() == _golden(case, kind), kind


# ---- the stage looks at one read at a time: the batched, sliced and multi-process modes -------------------------------------------
def _sum_totals(stderr):
    tot = [0, 0, 0]
    for l in stderr.splitlines():
        m = re.search(r"PCR 5' primer correction: (\d+) reads with (\d+) bases corrected, (\d+) reads with excessive", l)
        if m:
            tot = [t + int(m.group(k + 1)) for k, t in enumerate(tot)]
    return tot


def test_batched_mode_gives_the_same_sam(tmp_path):
    out = str(tmp_path / "b.sam")
    cmd = [a for a in _command(tmp_path, "s1_p3_M1", out, ["-b", "1"]) if a != "-M1"]  # (-M1 is written by the pipelined modes)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    want = _body(_unxz(tmp_path, "primer_s1_p3_M1.sam.xz"))
    assert _same_alignments(_body(out), [l for l in want if "YU:Z:" not in l])
    assert _sum_totals(p.stderr) == CASES["s1_p3_M1"]["totals"]


def test_sliced_runs_merge_to_the_same_sam(tmp_path):
    parts, tot = [], [0, 0, 0]
    for i in (0, 1):
        parts.append(str(tmp_path / ("s%d.sam" % i)))
        cmd = [a for a in _command(tmp_path, "s1_p3_M1", parts[-1], ["-S", "%d/2" % i]) if a != "-M1"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        tot = [a + b for a, b in zip(tot, _sum_totals(p.stderr))]
    out = str(tmp_path / "m.sam")
    p = subprocess.run([K4MERGE, out] + parts, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    want = _body(_unxz(tmp_path, "primer_s1_p3_M1.sam.xz"))
    assert _same_alignments(_body(out), [l for l in want if "YU:Z:" not in l]) and tot == CASES["s1_p3_M1"]["totals"]


def test_one_rank_multi_gpu_mode_gives_the_same_sam(tmp_path):
    out = str(tmp_path / "g.sam")
    p = subprocess.run([a for a in _command(tmp_path, "s1_p3_M1", out, ["-G", "0"]) if a != "-M1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    want = _body(_unxz(tmp_path, "primer_s1_p3_M1.sam.xz"))
    got = _body(out)
    n_acc = sum(1 for l in want if "YU:Z:" not in l)
    assert _same_alignments([l for l in got if "YU:Z:" not in l], want[:n_acc])
    assert _sum_totals(p.stderr) == CASES["s1_p3_M1"]["totals"]


# ---- the entry point on crafted records --------------------------------------------------------------------------------------------
N_CRAFTED = 25_000  # per max_subs: 100 000 records over the four of them


@pytest.fixture(scope="module")
def g1():
    import kit4b_amd

    kit4b_amd.lib()
    assert kit4b_amd.RESULT_DTYPE == primer_craft.RESULT_DTYPE and kit4b_amd.HIT_DTYPE == primer_craft.HIT_DTYPE
    assert kit4b_amd.PE_READ_DTYPE == primer_craft.PE_READ_DTYPE
    x = kit4b_amd.SfxIndex.open(os.path.join(GOLDEN, "g1.sfx"))
    yield x
    x.close()


@pytest.fixture(scope="module")
def genome():
    return synth.golden_genome()


def _dev(a, pad=0):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    return torch.cat([t, torch.zeros(pad, dtype=torch.uint8, device="cuda")]) if pad else t


@pytest.mark.parametrize("max_subs", [0, 1, 2, 5])
def test_stage_equals_the_restatement(g1, genome, max_subs):
    import torch

    _, chroms = genome
    s = primer_craft.craft(chroms, N_CRAFTED, 0x6B00 + max_subs)
    e = primer_craft.expected(s, max_subs, chroms)
    assert e["totals"][0] > 1000 and e["totals"][1] > e["totals"][0] and e["totals"][2] > 1000
    n = len(s["lens"])
    d_reads, d_offs, d_lens = _dev(s["reads"], 64), _dev(s["offs"]), _dev(s["lens"])
    d_rr, d_hits = _dev(s["rr"]), _dev(s["hits"])
    got = g1.pcr5_primer_correct(max_subs, n, 1, d_reads, d_offs, d_lens, d_rr=d_rr, d_hits=d_hits, stream=torch.cuda.current_stream().cuda_stream)
    assert list(got) == e["totals"]
    reads = d_reads.cpu().numpy()
    assert np.array_equal(reads[:len(s["reads"])], e["reads"]) and not reads[len(s["reads"]):].any()  # every byte of the read buffer
    rr, hits = d_rr.cpu().numpy().view(primer_craft.RESULT_DTYPE), d_hits.cpu().numpy().view(primer_craft.HIT_DTYPE)
    for k in ("low_mm", "nar", "num_hits", "inst", "hit_rslt", "nxt_mm"):
        assert np.array_equal(rr[k], e["rr"][k]), k
    assert np.array_equal(hits.view(np.uint8), e["hits"].view(np.uint8))  # mismatches; everything else as it was
    # idempotence: a second call on the result changes nothing and counts no correction
    again = g1.pcr5_primer_correct(max_subs, n, 1, d_reads, d_offs, d_lens, d_rr=d_rr, d_hits=d_hits)
    assert list(again) == [0, 0, 0]
    assert np.array_equal(d_reads.cpu().numpy(), reads) and np.array_equal(d_rr.cpu().numpy().view(np.uint8), rr.view(np.uint8))
    assert np.array_equal(d_hits.cpu().numpy(), hits.view(np.uint8))


def test_stage_on_the_pe_record_form(g1, genome):
    _, chroms = genome
    s = primer_craft.craft(chroms, N_CRAFTED, 0x6B10)
    e = primer_craft.expected(s, 1, chroms)
    n = len(s["lens"])
    want = primer_craft.as_pe(e["rr"], e["hits"])
    want["pe_aligned"] = s["rr"]["nar"] == 1  # (FlgPEAligned stays on a rejected mate)
    d_pe = _dev(primer_craft.as_pe(s["rr"], s["hits"]))
    d_reads, d_offs, d_lens = _dev(s["reads"], 64), _dev(s["offs"]), _dev(s["lens"])
    got = g1.pcr5_primer_correct(1, n, 1, d_reads, d_offs, d_lens, d_pe=d_pe)
    assert list(got) == e["totals"] and e["totals"][0] > 1000 and e["totals"][2] > 1000
    assert np.array_equal(d_pe.cpu().numpy(), want.view(np.uint8))
    assert np.array_equal(d_reads.cpu().numpy()[:len(s["reads"])], e["reads"])
    assert list(g1.pcr5_primer_correct(1, n, 1, d_reads, d_offs, d_lens, d_pe=d_pe)) == [0, 0, 0]
    assert np.array_equal(d_pe.cpu().numpy(), want.view(np.uint8))


def test_stage_with_nothing_to_do(g1, genome):
    import kit4b_amd

    _, chroms = genome
    s = primer_craft.craft(chroms, 2000, 0x6B20)
    d_reads, d_offs, d_lens, d_rr, d_hits = _dev(s["reads"], 64), _dev(s["offs"]), _dev(s["lens"]), _dev(s["rr"]), _dev(s["hits"])
    call = lambda subs, n, klen: list(g1.pcr5_primer_correct(subs, n, 1, d_reads, d_offs, d_lens, d_rr=d_rr, d_hits=d_hits, klen=klen))  # noqa: E731
    assert call(1, 0, 12) == [0, 0, 0] and call(1, len(s["lens"]), 0) == [0, 0, 0]
    assert np.array_equal(d_rr.cpu().numpy(), s["rr"].view(np.uint8)) and np.array_equal(d_reads.cpu().numpy()[:len(s["reads"])], s["reads"])
    for subs, klen in ((16, 12), (-1, 12), (1, 13)):
        with pytest.raises(kit4b_amd.K4Error) as err:
            call(subs, len(s["lens"]), klen)
        assert err.value.code == -100
