"""Golden outputs of kalign's alignment statistics files (`-O <file>`: CKAligner::WriteSubDist / WriteBasicCountStats /
ReportTargHitCnts and the insert size file of ProcessPairedEnds, ngskit4b/KAligner.cpp:6469-6525, 4159-4300, 5458-5712, 3092-3146)
from the REAL reference front end (`oracle/_ref/ngskit4b`, built by `make -C oracle ngskit4b`), run with ONE thread.

    python tests/golden/make_golden_stats.py

Per case (stats_cases.json): the command line, the reads, the NAR histogram of the reference's log, and what it wrote: the SAM
(stats_<case>.sam.xz), the main statistics file (.main.xz), <stem>.AlignCntsDist.csv (.cnts.xz; absent when the reference wrote
none) and for PE <stem>.GlobalPEInsertDist.csv (.peins.xz).  Reads come from the sets other golden scripts made, plus three small
sets made here: reads of the first two sequences only (the index's last entries get no alignment), reads of the first and the
fourth sequence (a gap in the middle) and random reads (nothing aligns).  The script checks that the cases exercise what they
are there for.  Data only.
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

# name: (index, reads (-i[, -u]), kalign args)
CASES = {
    "se_s2": ("g1", ["pcrdup_a.fa.xz"], ["-s2"]),
    "se_g0": ("g1", ["qual_se_g0.fq.xz"], ["-s2", "-g0"]),
    "se_r2_R8": ("g2", ["sam_se_cluster.fa.xz"], ["-s2", "-r2", "-R8"]),
    "se_r3_R8": ("g2", ["sam_se_cluster.fa.xz"], ["-s2", "-r3", "-R8"]),
    "se_c50": ("g3", ["pcrdup_c.fa.xz"], ["-s2", "-c50"]),
    "se_x5": ("g1", ["pcrdup_a.fa.xz"], ["-s3", "-x5"]),
    "se_a12_A3000": ("g3", ["sam_se_all_120.fa.xz"], ["-s2", "-a12", "-A3000"]),
    "se_k20": ("g1", ["pcrdup_a.fa.xz"], ["-s2", "-k20"]),
    "pe_u1": ("g1", ["sam_pe_u1_1.fa.xz", "sam_pe_u1_2.fa.xz"], ["-s2", "-U1", "-d200", "-D600"]),
    "pe_u2": ("g1", ["sam_pe_u1_1.fa.xz", "sam_pe_u1_2.fa.xz"], ["-s2", "-U2", "-d200", "-D600"]),
    "pe_u3": ("g1", ["sam_pe_u1_1.fa.xz", "sam_pe_u1_2.fa.xz"], ["-s2", "-U3", "-d200", "-D600"]),
    "se_tail": ("g1", ["stats_tail.fa.xz"], ["-s2"]),
    "se_gap": ("g1", ["stats_gap.fa.xz"], ["-s2"]),
    "se_none": ("g1", ["stats_none.fa.xz"], ["-s2"]),
}


def hist_of(log):
    hist = {}
    for line in open(log):
        m = re.search(r"\)\s+(\d+) \((\w\w)\) ", line)
        if m:
            hist[m.group(2)] = int(m.group(1))
    return hist


def xz(src, dst):
    with open(src, "rb") as f, lzma.open(os.path.join(HERE, dst), "wb", preset=9) as g:
        g.write(f.read())


def unxz(name, dst):
    with lzma.open(os.path.join(HERE, name)) as f, open(dst, "wb") as g:
        shutil.copyfileobj(f, g)
    return dst


def clips(cigar):
    """(leading soft clip, trailing soft clip, other operations than M / S) of a CIGAR"""
    ops = re.findall(r"(\d+)([A-Z])", cigar)
    lead = int(ops[0][0]) if ops[0][1] == "S" else 0
    trail = int(ops[-1][0]) if len(ops) > 1 and ops[-1][1] == "S" else 0
    return lead, trail, any(o not in "MS" for _, o in ops)


def bands_live(main_text):
    """quality bands with a non-zero instance count in a main statistics file"""
    rows = main_text.split('"Phred Score Instances"')[1].split('"Aligner Induced Subs"')[0].strip().split("\n")[1:]
    return sum(1 for r in rows if any(int(x) for x in r.split(",")[2:]))


def main():
    _, g1 = synth.golden_genome()
    with tempfile.TemporaryDirectory() as tmp:
        sfx = {"g1": os.path.join(HERE, "g1.sfx"), "g2": unxz("g2.sfx.xz", os.path.join(tmp, "g2.sfx")),
               "g3": unxz("g3.sfx.xz", os.path.join(tmp, "g3.sfx"))}
        # the three small sets of this script
        tail = synth.make_reads(g1[:2], 300, 100, seed=0x57A1, sub_lambda=1.0)[0]
        gap = synth.make_reads([g1[0]], 200, 100, seed=0x57A2, sub_lambda=1.0)[0] + synth.make_reads([g1[3]], 60, 60, seed=0x57A3, sub_lambda=0.5)[0]
        rng = np.random.default_rng(0x57A4)
        none = [rng.integers(0, 4, 100).astype(np.uint8) for _ in range(120)]
        for name, reads in (("stats_tail.fa", tail), ("stats_gap.fa", gap), ("stats_none.fa", none)):
            synth.write_fasta(os.path.join(tmp, name), reads)
            xz(os.path.join(tmp, name), name + ".xz")
        meta, texts = {}, {}
        for name, (index, reads, args) in CASES.items():
            files = []
            for flag, r in zip(("-i", "-u"), reads):
                files += [flag, unxz(r, os.path.join(tmp, r[:-3]))]
            out = os.path.join(tmp, name + ".sam")
            stats = os.path.join(tmp, name + ".stats.csv")
            log = out + ".log"
            subprocess.run([NGS, "kalign", "-I", sfx[index], "-o", out, "-O", stats, "-T", "1", "-F", log] + args + files, check=True,
                           capture_output=True, timeout=900)
            side = {"main": stats, "cnts": os.path.join(tmp, name + ".stats.AlignCntsDist.csv"),
                    "peins": os.path.join(tmp, name + ".stats.GlobalPEInsertDist.csv")}
            m = dict(index=index, reads=reads, args=args, nar=hist_of(log), files=[])
            xz(out, "stats_%s.sam.xz" % name)
            for key, path in side.items():
                if os.path.exists(path):
                    xz(path, "stats_%s.%s.xz" % (name, key))
                    m["files"].append(key)
                    texts[name, key] = open(path).read()
            texts[name, "sam"] = open(out).read()
            meta[name] = m
            print(name, m["nar"].get("AA"), m["files"])
        # ---- the cases exercise what they are there for -------------------------------------------------------------------------
        assert bands_live(texts["se_g0", "main"]) > 1, "se_g0: one quality band only"
        assert bands_live(texts["se_s2", "main"]) == 1
        for name in ("se_r2_R8", "se_r3_R8"):
            row = texts[name, "main"].split("\n")[2].split(",")[3:]
            assert len(row) == 8 and sum(int(x) > 0 for x in row) >= 2, (name, row)
        for name in ("se_c50", "se_x5"):  # a '-' alignment trimmed differently at its two ends (TrimLeft != TrimRight)
            n = 0
            for l in texts[name, "sam"].splitlines():
                if l.startswith("@"):
                    continue
                f = l.split("\t")
                lead, trail, _ = clips(f[5])
                n += (int(f[1]) & 16) != 0 and lead != trail
            assert n > 0, name
        assert any(clips(l.split("\t")[5])[2] for l in texts["se_a12_A3000", "sam"].splitlines() if not l.startswith("@")), "no two-segment read"
        tot = {u: sum(int(l.split(",")[1]) for l in texts["pe_" + u, "peins"].splitlines()) for u in ("u1", "u2", "u3")}
        assert tot["u1"] > tot["u2"] > 0 and tot["u3"] > tot["u2"], tot  # pairs accepted through a rescued mate (:3408 / :3511)
        zero_mid, zero_end = ",0,0.0,0" + ",0.0" * 64 + ",0\n", ",0,0.0,0" + ",0" * 64 + ",0\n"
        assert zero_end in texts["se_tail", "cnts"] and zero_mid in texts["se_gap", "cnts"] and zero_end in texts["se_gap", "cnts"]
        assert texts["se_none", "main"] == "" and ("se_none", "cnts") not in texts and meta["se_none"]["nar"].get("AA") == 0
        assert "DP" in meta["se_k20"]["nar"] and meta["se_k20"]["nar"]["DP"] > 100
        with open(os.path.join(HERE, "stats_cases.json"), "w") as f:  # one case per line
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(meta.items())) + "\n}\n")


if __name__ == "__main__":
    main()
