"""kalign's contaminant flank trimming (`-H`) on the device: k4_contam_trims_dev against the brute-force model (tests/contam_ref.py) on
the crafted cases of tests/contam_craft.py and on 20 000 random reads, and `k4align -H` against the SAM files the reference wrote
(tests/golden/make_golden_contam.py) -- pipelined, in batches (-b), in slices (-S i/N + k4merge) -- and against runs over reads
trimmed beforehand by the model (-M1, -M3)."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import contam_craft as K
import contam_ref as R
import kit4b_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
K4ALIGN, K4MERGE = os.path.join(ROOT, "kit4b_amd", "k4align"), os.path.join(ROOT, "kit4b_amd", "k4merge")
CASES = json.load(open(os.path.join(GOLDEN, "contam_cases.json")))


@pytest.fixture(scope="module")
def ix():
    x = kit4b_amd.SfxIndex.open(os.path.join(GOLDEN, "g1.sfx"))
    yield x
    x.close()


def _table(tmp_path, text):
    p = tmp_path / "c.fa"
    p.write_bytes(text)
    return kit4b_amd.load_contaminants(str(p)), R.parse_contaminants(text)


def test_crafted_cases_match_the_model(ix, tmp_path):
    groups = {}
    for text, t5, t3, r1, r2, note in K.cases():
        groups.setdefault((text, t5, t3, r2 is not None), []).append((r1, r2, note))
    n_checked = 0
    for (text, t5, t3, pe), cs in groups.items():
        tbl, ent = _table(tmp_path, text)
        reads1 = [np.array(c[0], dtype=np.uint8) for c in cs]
        reads2 = [np.array(c[1], dtype=np.uint8) for c in cs] if pe else None
        c5, c3, tot = ix.contaminant_trims(tbl, reads1, reads2, trim5=t5, trim3=t3)
        want = [[R.read_trims(ent, c[e], e == 1, t5, t3) for e in range(2 if pe else 1)] for c in cs]
        for k, (c, w) in enumerate(zip(cs, want)):
            for e in range(len(w)):
                at = 2 * k + e if pe else k
                assert (int(c5[at]), int(c3[at])) == w[e], (c[2], e)
                n_checked += 1
            exp = K.expect(c[2])
            if exp:
                assert w[0][0] == exp[0] and (exp[1] is None or w[0][1] == exp[1]), c[2]
        assert tot == (sum(w[0][0] > 0 for w in want), sum(w[0][1] > 0 for w in want), sum(w[1][0] > 0 for w in want) if pe else 0,
                       sum(w[1][1] > 0 for w in want) if pe else 0)
    assert n_checked > 250


def test_random_reads_match_the_model(ix, tmp_path):
    rng = np.random.default_rng(5)
    recs = [("r%d@%s" % (k, code), [int(x) for x in rng.choice(5, int(rng.integers(4, 61)), p=[.245, .245, .245, .245, .02])])
            for k, code in enumerate(["1", "3", "13", "57", "1357", "5", "7", "12345678", "24", "68", "1", "3"] * 3)]
    text = K.fasta(recs)
    tbl, ent = _table(tmp_path, text)
    for rl, n, t5, t3 in ((100, 12000, 0, 0), (37, 4000, 2, 0), (151, 4000, 0, 3)):
        reads = [rng.choice([0, 1, 2, 3, 4, 6], size=(n, rl), p=[.24, .24, .24, .24, .03, .01]).astype(np.uint8) for _ in range(2)]
        for e, rd in enumerate(reads):  # a third of the reads carry a piece of a contaminant of their class on either end
            for five in (True, False):
                mine = [b for c, b, _, _ in ent if c == (0 if five else 2) + e]
                for i in range(0, n, 3):
                    b = mine[int(rng.integers(len(mine)))]
                    L = int(rng.integers(1, min(len(b), rl // 2) + 1))
                    if five:
                        rd[i, :L] = b[len(b) - L:]
                    else:
                        rd[i, rl - L:] = b[:L]
                    if rng.random() < 0.5:
                        at = int(rng.integers(L)) if five else rl - 1 - int(rng.integers(L))
                        rd[i, at] = (rd[i, at] + 1) % 4
        flat = lambda a: (a.reshape(-1), np.arange(n, dtype=np.uint64) * rl, np.full(n, rl, np.uint32))  # noqa: E731
        c5, c3, tot = ix.contaminant_trims(tbl, flat(reads[0] | 0x50), flat(reads[1]), trim5=t5, trim3=t3)
        for e in range(2):
            w5 = np.maximum(R.match_many(ent, e, t5 + 1, reads[e]) - t5, 0)
            w3 = np.maximum(R.match_many(ent, 2 + e, t3 + 1, reads[e]) - t3, 0)
            assert np.array_equal(c5[e::2], w5) and np.array_equal(c3[e::2], w3), (rl, e)
            assert tot[2 * e] == int((w5 > 0).sum()) and tot[2 * e + 1] == int((w3 > 0).sum())
        for i in range(0, n, 997):  # the array model against the plain one
            assert max(R.match(ent, 0, t5 + 1, list(reads[0][i])) - t5, 0) == int(c5[2 * i])


def _files(case):
    return ["-i", os.path.join(GOLDEN, "contam_se.fq")] if case.startswith("se") else \
        ["-i", os.path.join(GOLDEN, "contam_pe_1.fa"), "-u", os.path.join(GOLDEN, "contam_pe_2.fa")]


def _run(out, args):
    p = subprocess.run([K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-o", str(out)] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


def _split(text):
    lines = text.splitlines()
    head = [l for l in lines if l.startswith("@") and not l.startswith("@PG")]
    body = [l for l in lines if not l.startswith("@")]
    return head, [l for l in body if "YU:Z:" not in l], sorted(l for l in body if "YU:Z:" in l)


def _golden(case):
    return _split(lzma.open(os.path.join(GOLDEN, "contam_%s.sam.xz" % case)).read().decode())


def _totals(stderr, pe):
    import re

    got = [int(x) for m in re.finditer(r"k4align: (\d+) 5' and (\d+) 3' contaminant trimmed (?:SE|PE1|PE2) reads", stderr) for x in m.groups()]
    assert len(got) == (4 if pe else 2), stderr
    return got


@pytest.mark.parametrize("case", sorted(CASES))
def test_k4align_writes_the_reference_sam(tmp_path, case):
    """-M1: every loaded read with the sequence and the qualities the reference stored; the unaligned records follow the alignments
    grouped by NAR, within a code in an order the reference leaves undefined"""
    out = tmp_path / "o.sam"
    p = _run(out, CASES[case]["args"] + ["-M1", "-H", os.path.join(GOLDEN, "contam.fa")] + _files(case))
    assert _split(out.read_text()) == _golden(case)
    assert _totals(p.stderr, case.startswith("pe")) == CASES[case]["totals"]


@pytest.mark.parametrize("case", ["se_y3_Y2", "pe"])
def test_batches_and_slices_write_the_same_alignments(tmp_path, case):
    """-b (three batches and more) and -S 1/2 + -S 2/2 merged: the accepted alignments of the reference's SAM, and the same totals"""
    args = CASES[case]["args"] + ["-H", os.path.join(GOLDEN, "contam.fa")] + _files(case)
    head, aligned, _ = _golden(case)
    one = tmp_path / "one.sam"
    p = _run(one, args)
    assert _split(one.read_text())[:2] == (head, aligned)
    # -b reads on in steps of a MiB at least and never across a file's end: the fixture's reads go in as four files per end
    split = []
    for flag, path in zip(_files(case)[::2], _files(case)[1::2]):
        lines = open(path).read().splitlines(True)
        per = 4 if path.endswith(".fq") else 2
        n_rec = len(lines) // per
        for q in range(4):
            part = tmp_path / ("%s_%d_%s" % (flag[1], q, os.path.basename(path)))
            part.write_text("".join(lines[per * (n_rec * q // 4):per * (n_rec * (q + 1) // 4)]))
            split += [flag, str(part)]
    b = tmp_path / "b.sam"
    pb = _run(b, CASES[case]["args"] + ["-H", os.path.join(GOLDEN, "contam.fa"), "-b", "0.004"] + split)
    assert int(pb.stderr.split(" batches)")[0].rsplit("(", 1)[1]) >= 3, pb.stderr
    assert _split(b.read_text())[:2] == (head, aligned)
    assert _totals(pb.stderr, case.startswith("pe")) == CASES[case]["totals"]
    parts, tot = [], None
    for i in range(2):
        parts.append(str(tmp_path / ("s%d.sam" % i)))
        ps = _run(parts[-1], args + ["-S", "%d/2" % i])
        t = _totals(ps.stderr, case.startswith("pe"))
        tot = t if tot is None else [x + y for x, y in zip(tot, t)]
    m = tmp_path / "m.sam"
    pm = subprocess.run([K4MERGE, str(m)] + parts, capture_output=True, text=True, timeout=120)
    assert pm.returncode == 0, pm.stderr
    got = _split(m.read_text())
    assert got[0] == head and sorted(got[1]) == sorted(aligned)
    assert tot == CASES[case]["totals"]


def _pretrimmed(tmp_path, trim5=0, trim3=0, nth=1):
    """the PE fixture's reads as contam_ref stores them (every n-th pair), for a run without -H"""
    ent = R.parse_contaminants(open(os.path.join(GOLDEN, "contam.fa"), "rb").read())
    recs = []
    for k in (1, 2):
        ls = open(os.path.join(GOLDEN, "contam_pe_%d.fa" % k)).read().split("\n")
        recs.append([(ls[i][1:], ls[i + 1]) for i in range(0, len(ls) - 1, 2)])
    res = R.load_reads(ent, [R.codes(s) for _, s in recs[0]], [R.codes(s) for _, s in recs[1]], trim5, trim3, 50, 500, nth)
    paths = [str(tmp_path / ("t%d.fa" % k)) for k in (1, 2)]
    for e, p in enumerate(paths):
        with open(p, "w") as f:
            for i, spans in res["kept"]:
                f.write(">%s\n%s\n" % (recs[e][i][0], recs[e][i][1][spans[e][0]:spans[e][1]]))
    return paths, res


def test_M1_and_sampling_equal_a_run_over_pretrimmed_reads(tmp_path):
    """-M1 with -#3 -y3 -Y2: the stage runs on the reads -# chose, in front of the end trims' arithmetic; every later report sees only the
    trimmed reads, so the run equals one over the reads the model trimmed (no -H, no -y / -Y, no -#)"""
    base = ["-s2", "-U2", "-d100", "-D800", "-M1"]
    a, b = tmp_path / "a.sam", tmp_path / "b.sam"
    pa = _run(a, base + ["-#3", "-y3", "-Y2", "-H", os.path.join(GOLDEN, "contam.fa")] + _files("pe"))
    (t1, t2), res = _pretrimmed(tmp_path, 3, 2, 3)
    assert len(res["kept"]) > 20
    _run(b, base + ["-i", t1, "-u", t2])
    assert _split(a.read_text()) == _split(b.read_text())
    assert _totals(pa.stderr, True) == res["totals"]


def test_M3_equals_a_run_over_pretrimmed_reads(tmp_path):
    ids = ["--experimentid", "e", "--readsetid", "r"]
    base = ["-s2", "-U2", "-d100", "-D800", "-M3"] + ids
    a, b = tmp_path / "a.pba", tmp_path / "b.pba"
    _run(a, base + ["-H", os.path.join(GOLDEN, "contam.fa")] + _files("pe"))
    (t1, t2), _ = _pretrimmed(tmp_path)
    _run(b, base + ["-i", t1, "-u", t2])
    assert a.read_bytes() == b.read_bytes() and a.stat().st_size > 0


def test_without_H_the_run_is_the_one_before(tmp_path):
    """no -H: the SAM of the existing golden case, and no word about contaminants"""
    reads = tmp_path / "se_s2.fa"
    reads.write_bytes(lzma.open(os.path.join(GOLDEN, "sam_se_s2.fa.xz")).read())
    out = tmp_path / "o.sam"
    p = _run(out, ["-s2", "-i", str(reads)])
    want = lzma.open(os.path.join(GOLDEN, "sam_se_s2.sam.xz")).read().decode()
    assert _split(out.read_text())[:2] == _split(want)[:2]
    assert "contaminant" not in p.stderr
