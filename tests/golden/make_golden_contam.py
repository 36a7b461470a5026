"""Goldens of kalign's contaminant flank trimming (`-H <file>`) from the REAL reference front end (`oracle/_ref/ngskit4b`, built by
`make -C oracle ngskit4b`), on the CPU, against tests/golden/g1.sfx.

    python tests/golden/make_golden_contam.py

Writes the crafted contaminants (contam.fa), the reads (contam_se.fq: FASTQ, run with -g0 so that the SAM shows the qualities going
with their bases; contam_pe_1.fa / contam_pe_2.fa), the SAM of every case with -M1 -- every loaded read is in it, so a read that is
missing was sloughed -- and contam_cases.json: per case its arguments and the four totals the reference logged.  SE and PE (-U2), with
-y3 -Y2 and without; contam_se_plain.sam.xz is the SE run WITHOUT -H (the qualities of the untrimmed reads).  Data only.

Every read of every -H SAM must differ from the same read of the run without -H in its sequence column (with a 5' contaminant loaded
every examined read loses at least one base): asserted here, so the fixtures cannot be met without the stage."""
import json
import lzma
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import synth  # noqa: E402

NGS = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")

CONTAMINANTS = """>adA@1 5' of SE / PE1
ACGTTGCAAGGCTTAACCGATCGTACGGATCCATGA
>adB@3 3' of SE / PE1
TTGACCAGTNCAGGATCAAGGCTAGCTAGGATC
>adC@24 5' and 3' of PE2
GGATTCAGCAATCGGCTAAGCTTAC
>adD@57 reverse complement onto both ends of SE / PE1
CCTAGGATACGATTACAGGCATCA
>plain
AAGGTTCCAAGTCGATCGGA
"""
CASES = {"se": ["-s2", "-g0"], "se_y3_Y2": ["-s2", "-g0", "-y3", "-Y2"], "pe": ["-s2", "-U2", "-d100", "-D800"],
         "pe_y3_Y2": ["-s2", "-U2", "-d100", "-D800", "-y3", "-Y2"]}


def flanked(rng, core, five, three):
    """the read with 5..20 bases of a contaminant of its 5' class in front and, mostly, 1..20 of its 3' class behind, now and then with a
    substitution"""
    parts = [core]
    for side, pool in ((0, five), (1, three)):
        if not pool or (side == 1 and rng.random() < 0.25):
            continue
        c = synth_codes(pool[int(rng.integers(len(pool)))])
        k = int(rng.integers(5, 21)) if side == 0 else int(rng.integers(1, 21))  # 5': beyond -y3 too, so that every read differs in every case
        piece = (c[len(c) - k:] if side == 0 else c[:k]).copy()
        piece[piece > 3] = rng.integers(0, 4, int((piece > 3).sum()))
        if k > 3 and rng.random() < 0.4:
            at = int(rng.integers(k))
            piece[at] = (piece[at] + 1) % 4
        parts = [piece] + parts if side == 0 else parts + [piece]
    return np.concatenate(parts).astype(np.uint8)


def synth_codes(s):
    return np.array(["ACGTN".index(ch) for ch in s], dtype=np.uint8)


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def main():
    assert os.path.exists(NGS), "needs oracle/_ref/ngskit4b (make -C oracle ngskit4b)"
    seqs = [l for l in CONTAMINANTS.split("\n") if l and not l.startswith(">")]
    a, b, c, d, plain = seqs
    five1, three1 = [a, rc(d), plain, rc(plain)], [b, rc(d)]
    five2, three2 = [c, plain, rc(plain)], [c]
    _, chroms = synth.golden_genome()
    rng = np.random.default_rng(20240)
    se = [flanked(rng, r[: int(rng.integers(40, 101))], five1, three1) for r in synth.make_reads(chroms, 160, 100, seed=611, n_prob=0.01)[0]]
    pe1, pe2, _ = synth.make_pe_reads(chroms, 120, 90, seed=612, frag_min=200, frag_max=500)
    pe1 = [flanked(rng, r[: int(rng.integers(45, 91))], five1, three1) for r in pe1]
    pe2 = [flanked(rng, r[: int(rng.integers(45, 91))], five2, three2) for r in pe2]
    with open(os.path.join(HERE, "contam.fa"), "w") as f:
        f.write(CONTAMINANTS)
    with open(os.path.join(HERE, "contam_se.fq"), "w") as f:
        for i, r in enumerate(se):
            qual = "".join(chr(33 + int(q)) for q in rng.integers(2, 41, len(r)))
            f.write("@se%04d\n%s\n+\n%s\n" % (i + 1, "".join("ACGTN"[x] for x in r), qual))
    synth.write_fasta(os.path.join(HERE, "contam_pe_1.fa"), pe1, prefix="pe")
    synth.write_fasta(os.path.join(HERE, "contam_pe_2.fa"), pe2, prefix="pe")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        def run(name, args, with_h):
            files = ["-i", os.path.join(HERE, "contam_se.fq")] if name.startswith("se") else \
                ["-i", os.path.join(HERE, "contam_pe_1.fa"), "-u", os.path.join(HERE, "contam_pe_2.fa")]
            sam, log = os.path.join(tmp, name + ".sam"), os.path.join(tmp, name + ".log")
            cmd = [NGS, "kalign", "-I", os.path.join(HERE, "g1.sfx"), "-o", sam, "-T", "2", "-F", log, "-M1"] + args + files
            subprocess.run(cmd + (["-H", os.path.join(HERE, "contam.fa")] if with_h else []), check=True, capture_output=True, timeout=600)
            totals = [int(m.group(1)) for m in re.finditer(r"total of (\d+) sequences PE1 sequences were [53]' contaminan?te? trimmed", open(log).read())]
            return open(sam, "rb").read(), totals

        def by_name(sam):
            out = {}
            for l in sam.split(b"\n"):
                if l and not l.startswith(b"@"):
                    f = l.split(b"\t")
                    out[(f[0], int(f[1]) & 0xC0)] = rc(f[9].decode()) if int(f[1]) & 16 else f[9].decode()
            return out

        for name, args in CASES.items():
            sam, totals = run(name, args, True)
            plain_sam, _ = run(name + "_plain", args, False)
            with_h, without = by_name(sam), by_name(plain_sam)
            assert with_h and all(k in without and without[k] != s for k, s in with_h.items()), name
            with lzma.open(os.path.join(HERE, "contam_%s.sam.xz" % name), "wb", preset=9) as g:
                g.write(sam)
            if name == "se":
                with lzma.open(os.path.join(HERE, "contam_se_plain.sam.xz"), "wb", preset=9) as g:
                    g.write(plain_sam)
            meta[name] = dict(args=args, totals=totals, n_reads=len(with_h), n_reads_plain=len(without))
            print(name, meta[name])
    json.dump(meta, open(os.path.join(HERE, "contam_cases.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
