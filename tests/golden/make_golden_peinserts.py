"""Golden outputs of kalign's per-target PE insert length distributions (`-3` / --petranslendist with `-O <file>`:
CKAligner::ReportPEInsertLenDist and MedianInsertLen, ngskit4b/KAligner.cpp:5255-5454) from the REAL reference front end
(`oracle/_ref/ngskit4b`, built by `make -C oracle ngskit4b`), run with ONE thread.

    python tests/golden/make_golden_peinserts.py

Per case (peinserts_cases.json): the index, the reads, the command line and what became of <-O file>.peinserts.csv: "rows" (the file
is peinserts_<case>.csv.xz), "empty" (created, nothing written: no read was accepted) or "absent" (an SE run: the option is off).
Reads come from the sets make_golden_sam.py made, plus two small sets made here: pairs whose fragments spread from 55 to 900 bases
over the three long sequences of g1 (its two short ones get none), and random pairs (nothing aligns).  The script checks that the
cases exercise what they are there for.  Data only.
"""
import json
import lzma
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import synth  # noqa: E402

NGS = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")
U1 = ["sam_pe_u1_1.fa.xz", "sam_pe_u1_2.fa.xz"]
C50 = ["sam_pe_c50_u1_1.fa.xz", "sam_pe_c50_u1_2.fa.xz"]
SPREAD = ["peinserts_spread_1.fa.xz", "peinserts_spread_2.fa.xz"]
NONE = ["peinserts_none_1.fa.xz", "peinserts_none_2.fa.xz"]

# name: (reads (-i[, -u]), kalign args); every case runs on g1 with -3 -O
CASES = {
    "pe_u1": (U1, ["-s2", "-U1", "-d200", "-D600"]),
    "pe_u2": (U1, ["-s2", "-U2", "-d200", "-D600"]),
    "pe_u3": (U1, ["-s2", "-U3", "-d200", "-D600"]),
    "pe_spread": (SPREAD, ["-s2", "-U1", "-d25", "-D1000"]),
    "pe_c50": (C50, ["-s2", "-c50", "-U1", "-d200", "-D600"]),
    "se_u1": (U1[:1], ["-s2"]),
    "pe_none": (NONE, ["-s2", "-U1", "-d200", "-D600"]),
}
ONLY_HERE = {"pe_c50_plain": (C50, ["-s2", "-U1", "-d200", "-D600"])}  # the comparison the -c50 case is checked against; not kept


def xz(src, dst):
    with open(src, "rb") as f, lzma.open(os.path.join(HERE, dst), "wb", preset=9) as g:
        g.write(f.read())


def unxz(name, dst):
    with lzma.open(os.path.join(HERE, name)) as f, open(dst, "wb") as g:
        shutil.copyfileobj(f, g)
    return dst


def rows_of(text):
    """{target name: [TargLen, TotPEs, Median, Mean, 52 columns]} of a .peinserts.csv"""
    lines = text.splitlines()
    assert lines[0].startswith('"TargSeq","TargLen","TotPEs","MedianInsertLen","MeanInsertLen","Insert <100bp","Insert 100bp"')
    assert lines[0].endswith('"Insert 590bp","Insert >600bp"') and lines[0].count(",") == 56
    return {l.split(",")[0].strip('"'): [int(x) for x in l.split(",")[1:]] for l in lines[1:]}


def equal_start_pairs(sam_text):
    """proper pairs whose two ends start at the same locus with different aligned lengths (SortPEHitMatch's comparator and the TLen
    rule are not symmetric there)"""
    seen, n = {}, 0
    for l in sam_text.splitlines():
        if l.startswith("@"):
            continue
        f = l.split("\t")
        if not int(f[1]) & 2:
            continue
        span = sum(int(k) for k, o in re.findall(r"(\d+)([A-Z])", f[5]) if o in "MDN")
        if f[0] in seen:
            pos, other = seen.pop(f[0])
            n += pos == f[3] and other != span
        else:
            seen[f[0]] = (f[3], span)
    return n


def main():
    _, g1 = synth.golden_genome()
    sfx = os.path.join(HERE, "g1.sfx")
    with tempfile.TemporaryDirectory() as tmp:
        a, b, _ = synth.make_pe_reads(g1, 3000, 50, seed=0x3E51, frag_min=55, frag_max=900, sub_lambda=0.5)
        rng = np.random.default_rng(0x3E52)
        rnd = [[rng.integers(0, 4, 100).astype(np.uint8) for _ in range(150)] for _ in range(2)]
        for name, reads in zip(SPREAD + NONE, (a, b, rnd[0], rnd[1])):
            synth.write_fasta(os.path.join(tmp, name[:-3]), reads)
            xz(os.path.join(tmp, name[:-3]), name)
        meta, texts, sams = {}, {}, {}
        for name, (reads, args) in list(CASES.items()) + list(ONLY_HERE.items()):
            files = []
            for flag, r in zip(("-i", "-u"), reads):
                files += [flag, unxz(r, os.path.join(tmp, r[:-3]))]
            out, stats = os.path.join(tmp, name + ".sam"), os.path.join(tmp, name + ".stats.csv")
            subprocess.run([NGS, "kalign", "-I", sfx, "-o", out, "-O", stats, "-3", "-T", "1", "-F", out + ".log"] + args + files, check=True,
                           capture_output=True, timeout=900)
            made = stats + ".peinserts.csv"  # (the suffix goes behind the whole name)
            sams[name] = open(out).read()
            if not os.path.exists(made):
                what = "absent"
            elif os.path.getsize(made) == 0:
                what = "empty"
            else:
                what, texts[name] = "rows", open(made).read()
                if name in CASES:
                    xz(made, "peinserts_%s.csv.xz" % name)
            if name in CASES:
                meta[name] = dict(index="g1", reads=reads, args=args, file=what)
            print(name, what, len(texts.get(name, "").splitlines()))
        # ---- the cases exercise what they are there for -------------------------------------------------------------------------
        rows = {k: rows_of(t) for k, t in texts.items()}
        names = ["%s" % n for n in synth.golden_genome()[0]]
        spread = rows["pe_spread"]
        assert len(spread) >= 3, spread.keys()
        cols = np.sum([r[4:] for r in spread.values()], axis=0)
        assert len(cols) == 52 and cols[0] > 0 and cols[25] > 0 and cols[51] > 0, cols
        assert set(spread) < set(names), (sorted(spread), names)  # a target of the index without a row
        tot = {u: sum(r[1] for r in rows["pe_" + u].values()) for u in ("u1", "u2", "u3")}
        assert tot["u1"] > tot["u2"] > 0, tot  # pairs accepted through a rescued mate
        assert any(rows["pe_c50"][k] != rows["pe_c50_plain"].get(k) for k in rows["pe_c50"]), "-c50 changes no row"
        assert meta["se_u1"]["file"] == "absent" and meta["pe_none"]["file"] == "empty"
        for name in CASES:
            assert equal_start_pairs(sams[name]) == 0, name
        with open(os.path.join(HERE, "peinserts_cases.json"), "w") as f:  # one case per line
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(meta.items())) + "\n}\n")


if __name__ == "__main__":
    main()
