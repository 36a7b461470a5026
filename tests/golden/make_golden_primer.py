"""Golden outputs of kalign's 5' PCR primer correction (`-6 <n>`, CKAligner::PCR5PrimerCorrect, ngskit4b/KAligner.cpp:2115-2226)
from the REAL reference front end (`oracle/_ref/ngskit4b`, built by `make -C oracle ngskit4b`), run with ONE thread.

    python tests/golden/make_golden_primer.py

Per case (primer_cases.json): the kalign / genpba arguments, what the reference wrote (primer_<case>.sam.xz / .bam, the SNP CSV of
-p5, the files of -O, the FASTA of -j, genpba's .pba and coverage WIG), its NAR histogram and the three totals of its "Completed
PCR 5' primer correction" log line.  For the restatement in tests/primer_ref.py: the names of the reads that are NL in the same run
under -M1 (primer_marks.json.xz), and one -M1 base run per distinct command line (primer_base_*.sam.xz): the same arguments without
-6 and the reports, aligned with -s<min(MaxSubs + n, 15)> -- the records the stage saw.  The flank autotrim (-x, forced by -A) runs
behind the stage, so a base run leaves it out where it can (`restate` is false for the -A case: no command line shows the untrimmed
records there).  Existing read sets and indexes only.  Data only.
"""
import json
import lzma
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

NGS = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")

A, P = ["pcrdup_a.fa.xz"], ["pcrdup_p_1.fa.xz", "pcrdup_p_2.fa.xz"]
# name: (reads (-i[, -u]), index, -s, -6, further arguments, output extension)
CASES = {
    "s2_p2": (A, "g1", 2, 2, [], "sam"),
    "s1_p3_M1": (A, "g1", 1, 3, ["-M1"], "sam"),
    "s0_p5": (A, "g1", 0, 5, [], "sam"),
    "s14_p5": (A, "g1", 14, 5, [], "sam"),  # the clamp to 15
    "s1_p3_k20_x5": (A, "g1", 1, 3, ["-k20", "-x5"], "sam"),
    "s1_p3_bam": (A, "g1", 1, 3, [], "bam"),
    "s1_p3_p5": (A, "g1", 1, 3, ["-p5"], "sam"),
    "s1_p3_O": (A, "g1", 1, 3, ["-O"], "sam"),
    "s1_p3_j": (A, "g1", 1, 3, ["-j"], "sam"),
    "seg_a12_A3000": (["sam_se_all_120.fa.xz"], "g3", 1, 3, ["-a12", "-A3000"], "sam"),  # two-segment reads are skipped
    "pe_u1": (P, "g1", 1, 3, ["-U1", "-d200", "-D600"], "sam"),
    "pe_u3_M1": (P, "g1", 1, 3, ["-U3", "-M1", "-d200", "-D600"], "sam"),
    "pba": (A, "g1", 1, 3, [], "pba"),  # ngskit4b genpba -w e1 -W r1
}
PBA_IDS = ["e1", "r1"]
REPORTS = ("-p", "-O", "-M", "-j")   # what only reports
BEHIND = ("-x",)                     # what runs behind the stage


def log_of(log):
    hist, totals = {}, None
    for line in open(log):
        m = re.search(r"\)\s+(\d+) \((\w\w)\) ", line)
        if m:
            hist[m.group(2)] = int(m.group(1))
        m = re.search(r"Completed PCR 5' primer correction, (\d+) reads with (\d+) bases corrected, (\d+) reads with excessive substitutions rejected", line)
        if m:
            totals = [int(m.group(k)) for k in (1, 2, 3)]
    return hist, totals


def xz(src, dst):
    with open(src, "rb") as f, lzma.open(os.path.join(HERE, dst), "wb", preset=9) as g:
        g.write(f.read())


def unxz(name, dst):
    with lzma.open(os.path.join(HERE, name)) as f, open(dst, "wb") as g:
        shutil.copyfileobj(f, g)
    return dst


def run(sub, sfx, out, args, files):
    cmd = [NGS, sub, "-I", sfx, "-o", out, "-T", "1", "-F", out + ".log"]
    for a in args:  # -O / -j take a file beside the output
        cmd += [a, out + (".stats.csv" if a == "-O" else ".none.fa")] if a in ("-O", "-j") else [a]
    subprocess.run(cmd + files, check=True, capture_output=True, timeout=900)
    return log_of(out + ".log")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        sfx = {"g1": os.path.join(HERE, "g1.sfx"), "g3": unxz("g3.sfx.xz", os.path.join(tmp, "g3.sfx"))}
        meta, marks, bases = {}, {}, {}
        for name, (reads, index, subs, primer, more, ext) in CASES.items():
            files = []
            for flag, r in zip(("-i", "-u"), reads):
                files += [flag, unxz(r, os.path.join(tmp, r[:-3]))]
            args = ["-s%d" % subs, "-6", str(primer)] + more
            out = os.path.join(tmp, "%s.%s" % (name, ext))
            if ext == "pba":
                hist, totals = run("genpba", sfx[index], out, args + ["-w", PBA_IDS[0], "-W", PBA_IDS[1]], files)
            else:
                hist, totals = run("kalign", sfx[index], out, args, files)
            m = dict(reads=reads, index=index, args=args, subs=subs, primer=primer, out=ext, nar=hist, totals=totals, files=[])
            if ext == "pba":
                m["ids"] = PBA_IDS
                xz(out, "primer_%s.pba.xz" % name)
                xz(os.path.join(tmp, name + ".covsegs.wig"), "primer_%s.covsegs.wig.xz" % name)  # AppendFileNameSuffix: the extension is replaced
            elif ext == "bam":
                shutil.copy(out, os.path.join(HERE, "primer_%s.bam" % name))
            else:
                xz(out, "primer_%s.sam.xz" % name)
            if "-p5" in more:
                xz(out + ".snp", "primer_%s.snp.xz" % name)  # (kalign -p without -S: <out>.snp)
            if "-j" in more:
                xz(out + ".none.fa", "primer_%s.none.xz" % name)
            if "-O" in more:
                for key, path in (("main", out + ".stats.csv"), ("cnts", out + ".stats.AlignCntsDist.csv")):
                    xz(path, "primer_%s.%s.xz" % (name, key))
                    m["files"].append(key)
            # the reads the stage rejected: the same run as -M1, the reports left out (kalign refuses -M1 with SNP calling)
            m1 = out
            if "-M1" not in more:
                m1 = os.path.join(tmp, name + ".m1.sam")
                _, t1 = run("kalign", sfx[index], m1, [a for a in args if not a.startswith(REPORTS)] + ["-M1"], files)
                assert t1 == totals, (name, t1, totals)
            marks[name] = sorted(l.split("\t", 2)[0] + "/" + str((int(l.split("\t", 2)[1]) >> 7) & 1) for l in open(m1) if l.endswith("YU:Z:NL\n"))
            # the run the stage started from: no -6, the inflated rate, nothing that runs behind the stage, every loaded read reported
            inflated = min(subs + primer, 15)
            bargs = ["-s%d" % inflated] + [a for a in more if not a.startswith(REPORTS + BEHIND)] + ["-M1"]
            bname = "primer_base_%s_%s.sam.xz" % (reads[0].split(".")[0], "_".join(a.lstrip("-") for a in bargs))
            if bname not in bases:
                base = os.path.join(tmp, name + ".base.sam")
                bases[bname] = run("kalign", sfx[index], base, bargs, files)[0]
                xz(base, bname)
            m["base"], m["base_nar"], m["base_subs"] = bname, bases[bname], inflated
            m["restate"] = not any(a.startswith("-A") for a in more)
            meta[name] = m
            print(name, {k: v for k, v in hist.items() if v}, totals, len(marks[name]))
        # ---- the cases exercise what they are there for ---------------------------------------------------------------------------
        for name, m in meta.items():
            if name == "s14_p5":
                # no read of the existing sets carries the 15 substitutions it would take to be over (14 * len + 50) / 100: the case
                # pins the clamp of the alignment rate alone -- its alignments are those of -s15 -- and the stage finds nothing to do
                assert m["base_subs"] == 15 and m["totals"] == [0, 0, 0] and m["nar"] == m["base_nar"], (name, m["totals"])
                continue
            assert m["totals"] and m["totals"][0] > 0 and m["totals"][2] > 0, (name, m["totals"])
        assert any(m["totals"][1] > m["totals"][0] for m in meta.values())
        with open(os.path.join(HERE, "primer_cases.json"), "w") as f:  # one case per line
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(meta.items())) + "\n}\n")
        with lzma.open(os.path.join(HERE, "primer_marks.json.xz"), "wt", preset=9) as f:
            json.dump(marks, f, sort_keys=True)


if __name__ == "__main__":
    main()
