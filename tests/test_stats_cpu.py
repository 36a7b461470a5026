"""kalign's alignment statistics files (`-O`) without a GPU: the restatement in tests/stats_ref.py reproduces, byte for byte, what
the reference binary wrote (tests/golden/make_golden_stats.py) from the reference's own SAM of the same run -- the multihit
distribution, which no SAM field carries, from the CPU oracle's alignment of the same reads -- and the argument rules of
`k4align -O`."""
import json
import lzma
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import stats_ref
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)
K4ALIGN = os.path.join(ROOT, "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "stats_cases.json")))
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
QSCORE = {33 + (q * 40) // 15: q for q in range(16)}  # the SAM quality character of a 4-bit score (KAligner.cpp:6120-6145)


def genome_of(index):
    """(names, sequences) of the index a case ran on"""
    if index == "g1":
        return synth.golden_genome()
    if index == "g2":
        return synth.cluster_genome()[:2]
    sys.path.insert(0, GOLDEN)
    from make_golden_ext import genome

    return genome()[:2]


def golden_text(case, key):
    p = os.path.join(GOLDEN, "stats_%s.%s.xz" % (case, key))
    return lzma.open(p, "rt").read() if os.path.exists(p) else None


def sam_records(case):
    """the accepted alignments of the case's golden SAM as restatement records, and the fragment lengths of its accepted pairs"""
    names, _ = genome_of(CASES[case]["index"])
    recs, frags = [], []
    for l in golden_text(case, "sam").splitlines():
        if l.startswith("@"):
            continue
        f = l.split("\t")
        flag = int(f[1])
        if flag & 4:
            continue
        ops = [(int(n), o) for n, o in re.findall(r"(\d+)([A-Z])", f[5])]
        lead = ops[0][0] if ops[0][1] == "S" else 0
        trail = ops[-1][0] if len(ops) > 1 and ops[-1][1] == "S" else 0
        segs = any(o not in "MS" for _, o in ops)
        minus = bool(flag & 16)
        seq = np.array([CODE[c] for c in f[9]], np.uint8)
        q = np.zeros(len(seq), np.uint8) if f[10] == "*" else np.array([QSCORE[ord(c)] for c in f[10]], np.uint8)
        if minus:  # SEQ / QUAL are those of the aligned strand: back to the read as it was loaded
            seq, q = stats_ref.COMP[seq[::-1]], q[::-1]
        tl, tr = (trail, lead) if minus else (lead, trail)
        first_m = [n for n, o in ops if o == "M"][0]
        mlen = len(seq) if not segs else first_m + lead  # (a two-segment hit is only counted per target: Seg[0] starts at POS - 1)
        recs.append(dict(nar=1, chrom=names.index(f[2]) + 1, loci=int(f[3]) - 1 - lead, mlen=mlen, strand="-" if minus else "+",
                         tl=tl if not segs else lead, tr=tr if not segs else 0, segs=segs, read=seq | (q << 4)))
        if (flag & 0x4A) == 0x42:  # first mate of a pair accepted as such (an orphan kept by -U3 / -U4 has its mate unmapped)
            frags.append(abs(int(f[8])))
    return recs, frags


def multi_hit_of(case):
    """m_MultiHitDist of an SE case: the CPU oracle's AlignRead over the case's reads"""
    from oracle_bindings import Oracle

    import samutil

    meta = CASES[case]
    O = Oracle()
    sfx = os.path.join(GOLDEN, meta["index"] + ".sfx")
    tmp = None
    if not os.path.exists(sfx):
        import tempfile

        tmp = tempfile.NamedTemporaryFile(suffix=".sfx")
        tmp.write(lzma.open(sfx + ".xz").read())
        tmp.flush()
        sfx = tmp.name
    h = O.open(sfx)
    O.set_max_iter(h, 5000)
    _, reads = samutil.read_fasta_xz(os.path.join(GOLDEN, meta["reads"][0]))
    max_ml = int([a for a in meta["args"] if a.startswith("-R")][0][2:])
    r = O.kalign_batch(h, reads, max_subs=2, max_ml=max_ml, pe_mode=0)
    O.close(h)
    return stats_ref.multi_hit_dist(r["out"]["hit_rslt"], r["out"]["inst"]), max_ml


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_reproduces_the_reference_files(case):
    meta = CASES[case]
    names, chroms = genome_of(meta["index"])
    chroms = [np.asarray(c, np.uint8) for c in chroms]
    recs, frags = sam_records(case)
    assert len(recs) == meta["nar"]["AA"]
    passes = 2 if any(a.startswith("-A") for a in meta["args"]) else 1
    st = stats_ref.collect(recs, chroms, max(max((len(r["read"]) for r in recs), default=1), 1), passes)
    ml_mode = int(([a for a in meta["args"] if a.startswith("-r")] or ["-r0"])[0][2:])
    multi, max_multi = (multi_hit_of(case) if ml_mode else (None, 0))
    assert stats_ref.main_text(st, ml_mode, max_multi, multi) == golden_text(case, "main")
    n_reads = sum(meta["nar"].values())  # every loaded read carries one NAR
    assert stats_ref.cnts_text(st, names, [len(c) for c in chroms], n_reads) == golden_text(case, "cnts")
    if len(meta["reads"]) == 2:
        d = np.zeros(stats_ref.PAIR_MAX_LEN + 1, np.uint64)
        for x in frags:
            d[x] += 1
        assert stats_ref.peins_text(d) == golden_text(case, "peins")
        assert len(frags) > 1000
    else:
        assert golden_text(case, "peins") is None


def test_goldens_cover_what_they_are_there_for():
    live = lambda t: sum(1 for r in t.split('"Phred Score Instances"')[1].split('"Aligner')[0].strip().split("\n")[1:]  # noqa: E731
                         if any(int(x) for x in r.split(",")[2:]))
    assert live(golden_text("se_g0", "main")) > 1
    for case in ("se_c50", "se_x5"):
        assert any(r["strand"] == "-" and r["tl"] != r["tr"] for r in sam_records(case)[0]), case
    assert any(r["segs"] for r in sam_records("se_a12_A3000")[0])
    assert golden_text("se_none", "main") == "" and golden_text("se_none", "cnts") is None
    tot = {u: sum(int(l.split(",")[1]) for l in golden_text("pe_" + u, "peins").splitlines()) for u in ("u1", "u2", "u3")}
    assert tot["u1"] > tot["u2"] and tot["u3"] > tot["u2"]  # the rescued pairs
    assert ",0,0.0,0" + ",0.0" * 64 + ",0\n" in golden_text("se_gap", "cnts") and ",0,0.0,0" + ",0" * 64 + ",0\n" in golden_text("se_tail", "cnts")


# ---- the argument rules of `k4align -O` ---------------------------------------------------------------------------------------
def _k4align(*args):
    return subprocess.run([K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-o", "/dev/null", "-i", os.path.join(GOLDEN, "names.fa")] + list(args),
                          capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra", [["-b", "1"], ["-S", "0/2"], ["-G", "0"], ["-Z"]])
def test_O_needs_the_whole_run(extra, tmp_path):
    p = _k4align("-O", str(tmp_path / "st.csv"), *extra)
    assert p.returncode == 1 and "-O counts over all reads of the run" in p.stderr
    assert not os.path.exists(str(tmp_path / "st.csv"))


def test_O_with_r5_is_not_built(tmp_path):
    p = _k4align("-O", str(tmp_path / "st.csv"), "-r5", "-R8")
    assert p.returncode == 3 and "not built" in p.stderr


def test_usage_names_the_option():
    p = subprocess.run([K4ALIGN], capture_output=True, text=True, timeout=60)
    assert "-O stats.csv" in p.stderr
