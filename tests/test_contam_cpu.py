"""kalign's contaminant flank trimming (`-H`) without a device: (a) the brute-force model tests/contam_ref.py against the SAM files the
reference wrote (tests/golden/make_golden_contam.py); (b) the host rule k4_contam_match_host against the model; (c) the loader
k4_load_contaminants; (d) what `k4align -H` says and leaves behind when the file is missing, refused or holds a vector record."""
import gzip
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import contam_craft as K
import contam_ref as R
import kit4b_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
K4ALIGN = os.path.join(ROOT, "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "contam_cases.json")))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(kit4b_amd.LIB_PATH) or not os.path.exists(K4ALIGN):
        kit4b_amd.build()


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def _sam_reads(name):
    """(read name, end 0 / 1) -> (sequence, qualities) as loaded (a Crick alignment turned back)"""
    out = {}
    for l in lzma.open(os.path.join(GOLDEN, name)).read().decode().splitlines():
        if l and not l.startswith("@"):
            f = l.split("\t")
            flag = int(f[1])
            out[(f[0], 1 if flag & 128 else 0)] = (_rc(f[9]), f[10][::-1]) if flag & 16 else (f[9], f[10])
    return out


def _fixture_reads(case):
    if case.startswith("se"):
        ls = open(os.path.join(GOLDEN, "contam_se.fq")).read().split("\n")
        return [[(ls[i][1:], ls[i + 1]) for i in range(0, len(ls) - 1, 4)]]
    ends = []
    for k in (1, 2):
        ls = open(os.path.join(GOLDEN, "contam_pe_%d.fa" % k)).read().split("\n")
        ends.append([(ls[i][1:].split()[0], ls[i + 1]) for i in range(0, len(ls) - 1, 2)])
    return ends


# ---- (a) the model against the reference's own runs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_model_reproduces_the_reference_sam(case):
    args = CASES[case]["args"]
    t5, t3 = (3, 2) if "-y3" in args else (0, 0)
    ent = R.parse_contaminants(open(os.path.join(GOLDEN, "contam.fa"), "rb").read())
    ends = _fixture_reads(case)
    res = R.load_reads(ent, *[[R.codes(s) for _, s in e] for e in ends], trim5=t5, trim3=t3)
    want = {}
    for i, spans in res["kept"]:
        for e, (a, b) in enumerate(spans):
            want[(ends[e][i][0], e)] = (ends[e][i][1][a:b], (a, b))
    got = _sam_reads("contam_%s.sam.xz" % case)
    assert set(got) == set(want)  # which reads were sloughed: -M1 reports every loaded read
    assert all(got[k][0] == want[k][0] for k in want)
    assert res["totals"][:len(CASES[case]["totals"])] == CASES[case]["totals"]
    assert res["under"] > 0 and len(want) == CASES[case]["n_reads"]
    if case == "se":  # the qualities go with their bases: the same slice of what the run without -H reports for the read
        plain = _sam_reads("contam_se_plain.sam.xz")
        assert all(got[k][1] == plain[k][1][want[k][1][0]:want[k][1][1]] for k in want) and len(plain) > len(got)


# ---- (b) the host rule against the model ---------------------------------------------------------------------------------------------
def _load(tmp_path, text, name="c.fa"):
    p = tmp_path / name
    p.write_bytes(text)
    return kit4b_amd.load_contaminants(str(p))


def test_host_rule_on_the_crafted_cases(tmp_path):
    tables = {}
    n = 0
    for text, t5, t3, r1, r2, note in K.cases():
        if text not in tables:
            tables[text] = (_load(tmp_path, text), R.parse_contaminants(text))
        tbl, ent = tables[text]
        for e, r in enumerate([r1] + ([r2] if r2 is not None else [])):
            rd = np.array(r, dtype=np.uint8)
            got = tuple(max(kit4b_amd.contam_match_host(tbl, c + e, t + 1, rd) - t, 0) for c, t in ((0, t5), (2, t3)))
            assert got == R.read_trims(ent, r, e == 1, t5, t3), (note, e)
            if e == 0 and K.expect(note):
                exp = K.expect(note)
                assert got[0] == exp[0] and (exp[1] is None or got[1] == exp[1]), note
            n += 1
    assert n > 250


def test_a_longer_read_than_2000_is_not_examined(tmp_path):
    c = [0, 1, 2, 3] * 10
    tbl = _load(tmp_path, K.fasta([("x@13", c)]))
    for rl, examined in ((19, False), (20, True), (2000, True), (2001, False)):
        rd = np.array((c + [0] * rl)[:rl - 20] + c[:20], dtype=np.uint8) if rl > 40 else np.array(c[40 - rl:], dtype=np.uint8)
        assert (kit4b_amd.contam_match_host(tbl, 0, 1, rd) > 0) == examined, rl
        assert (kit4b_amd.contam_match_host(tbl, 2, 1, rd) > 0) == examined, rl


def test_host_rule_on_random_cases(tmp_path):
    rng = np.random.default_rng(11)
    n = 0
    for t in range(40):
        recs = []
        for k in range(int(rng.integers(1, 12))):
            L = int(rng.integers(4, 201)) if rng.random() < 0.3 else int(rng.integers(4, 40))
            code = str(rng.choice(["", "@1", "@3", "@13", "@57", "@2468", "@12345678", "@", "@24"]))
            recs.append(("c%d%s" % (k, code), [int(x) for x in rng.choice(5, L, p=[.24, .24, .24, .24, .04])]))
        text = K.fasta(recs)
        try:
            ent = R.parse_contaminants(text)
        except R.Refused:  # (a palindrome on a class twice, as read and reverse complemented)
            with pytest.raises(kit4b_amd.K4Error):
                _load(tmp_path, text)
            continue
        tbl = _load(tmp_path, text)
        assert len(tbl) == len(ent)
        for q in range(100):
            rl = int(rng.choice([19, 20, 21, 63, 64, 65, 100, 150, 199, 200, 201, 300]))
            rd = rng.choice([0, 1, 2, 3, 4, 6], p=[.24, .24, .24, .24, .03, .01], size=rl).astype(np.uint8)
            cls = int(rng.integers(0, 4))
            mine = [b for c, b, _, _ in ent if c == cls]
            if mine and rng.random() < 0.7:
                b = mine[int(rng.integers(len(mine)))]
                L = int(rng.integers(1, min(len(b), rl) + 1))
                part = np.array(b[len(b) - L:] if cls < 2 else b[:L], dtype=np.uint8)
                base = 0 if cls < 2 else rl - L
                rd[base:base + L] = part
                for _ in range(int(rng.integers(0, 3))):
                    at = base + int(rng.integers(L))
                    rd[at] = (rd[at] + 1) % 4
            mo = int(rng.integers(0, 8))
            qual = np.uint8(int(rng.integers(0, 16)) << 4)  # the quality bits of a read byte do not count
            assert kit4b_amd.contam_match_host(tbl, cls, mo, rd | qual) == R.match(ent, cls, mo, [int(x) for x in rd]), (t, q)
            n += 1
    assert n > 3000


# ---- (c) the loader -----------------------------------------------------------------------------------------------------------------
def _classes(tbl):
    return sorted((int(e["cls"]), int(e["revcpl"])) for e in tbl)


def _unpack(e):
    """the bases of a table element, from its packed planes"""
    n, cls = int(e["len"]), int(e["cls"])
    out = []
    for k in range(n):
        p = 256 - n + k if cls < 2 else k
        bit = lambda w: int(w[p >> 6]) >> (p & 63) & 1  # noqa: E731
        out.append(4 if bit(e["nmask"]) else bit(e["p0"]) | bit(e["p1"]) << 1)
    return out


def test_loader_codes_and_defaults(tmp_path):
    seq = "ACGTTGCANGGC"
    for digit in "12345678":
        tbl = _load(tmp_path, (">n@%s\n%s\n" % (digit, seq)).encode())
        k = int(digit) - 1
        assert _classes(tbl) == [(k % 4, k // 4)]
        assert _unpack(tbl[0]) == (R.codes(seq) if k < 4 else [3 - b if b < 4 else b for b in reversed(R.codes(seq))])
    dflt = [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert _classes(_load(tmp_path, (">nocode some words\n%s\n" % seq).encode())) == dflt
    assert _classes(_load(tmp_path, (seq + "\n").encode())) == dflt                      # no descriptor at all
    assert _classes(_load(tmp_path, (">\n%s\n" % seq).encode())) == dflt                 # an empty one
    assert _classes(_load(tmp_path, (">name@\n%s\n" % seq).encode())) == dflt            # `@` with nothing behind it
    assert _classes(_load(tmp_path, (">name@9\n%s\n" % seq).encode())) == dflt           # 9 is no code: the name has none
    assert _classes(_load(tmp_path, (">n@1357\nacgt\nTTGC\n\n>m@28 x\n%s\n" % seq).encode())) == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1), (3, 1)]
    tbl = _load(tmp_path, (">a@1\n%s\n>b@1\n%s\n>c@1\n%s\n" % ("ACGT", "A" * 200, "ACGTA")).encode())
    assert [int(e["len"]) for e in tbl] == [200, 5, 4]  # by class and falling length
    gz = tmp_path / "c.fa.gz"
    gz.write_bytes(gzip.compress((">n@13\n%s\n" % seq).encode()))
    assert _classes(kit4b_amd.load_contaminants(str(gz))) == [(0, 0), (2, 0)]
    exc = R.parse_contaminants((">n@1357\nacgt\nTTGC\n\n>m@28 x\n%s\n" % seq).encode())
    assert sorted((c, int(rc)) for c, _, _, rc in exc) == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1), (3, 1)]


@pytest.mark.parametrize("text,code,sentence", [
    (b">short@1\nACG\n", -47, "LoadContamiantsFile: Sequence for 'short' outside of accepted length range 4..200"),
    (b">long@1\n" + b"ACGTA" * 40 + b"C\n", -47, "LoadContamiantsFile: Sequence for 'long' outside of accepted length range 4..200"),
    (b">gap@1\nACGT-ACGT\n", -47, "LoadContaminantsFile: Illegal base in gap sequence, only bases A,C,G,T,N accepted"),
    (b"", -100, "FinaliseContaminant: No Contaminants loaded"),
    (b">same@1\nACGTAC\n>same@1\nACGTAA\n", -47, "AddFlankContam: Contaminant name 'same' of overlap type 5'SE/PE1 duplicated with different sequences"),
    (b">a@3\nACGTAC\n>b@3\nACGTAC\n", -47, "AddFlankContam: Contaminant names 'b' and 'a' of overlap type 3'SE/PE1 with duplicated sequence"),
    (b">vec&1\n" + b"ACGT" * 30 + b"\n", -3, "vector contaminants ('&' codes: reads contained in 'vec') are not built"),
])
def test_loader_refusals(tmp_path, text, code, sentence):
    p = tmp_path / "bad.fa"
    p.write_bytes(text)
    with pytest.raises(kit4b_amd.K4Error) as e:
        kit4b_amd.load_contaminants(str(p))
    assert e.value.code == code and sentence in str(e.value)
    if code == -47 or code == -100:
        with pytest.raises(R.Refused):
            R.parse_contaminants(text)


def test_loader_takes_1600_entries_and_no_more(tmp_path):
    rng = np.random.default_rng(3)
    recs = [("e%d@12345678" % k, [int(x) for x in rng.integers(0, 4, 30)]) for k in range(201)]
    assert len(_load(tmp_path, K.fasta(recs[:200]))) == 1600
    with pytest.raises(kit4b_amd.K4Error) as e:
        _load(tmp_path, K.fasta(recs))
    assert e.value.code == -100 and "AddFlankContam: Too many flank contaminants (max allowed 1600) current contaminant is 'e200'" in str(e.value)
    with pytest.raises(kit4b_amd.K4Error) as e:
        kit4b_amd.load_contaminants(str(tmp_path / "missing.fa"))
    assert e.value.code == -90


# ---- (d) k4align -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,rc,sentence", [
    (None, 2, "Unable to open"),
    (b">short@1\nACG\n", 1, "LoadContamiantsFile: Sequence for 'short' outside of accepted length range 4..200"),
    (b">vec&15\n" + b"ACGT" * 30 + b"\n", 3, "vector contaminants ('&' codes: reads contained in 'vec') are not built"),
])
def test_k4align_turns_the_file_down_before_it_touches_a_device(tmp_path, text, rc, sentence):
    h = tmp_path / "h.fa"
    if text is not None:
        h.write_bytes(text)
    out = tmp_path / "o.sam"
    for flag in (["-H", str(h)], ["--contaminants", str(h)], ["--contaminants=" + str(h)]):
        p = subprocess.run([K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-o", str(out), "-i", os.path.join(GOLDEN, "contam_se.fq")] + flag,
                           capture_output=True, text=True, timeout=60)
        assert p.returncode == rc, p.stderr
        assert sentence in p.stderr
        assert ("Unable to load contaminate sequences file '%s'" % h in p.stderr) == (rc != 3)
        assert sorted(os.listdir(tmp_path)) == (["h.fa"] if text is not None else [])  # no output file is left behind
