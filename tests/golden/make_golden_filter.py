"""Golden outputs of kalign's loci base constraints (`-5 <file>`, CKAligner::IdentifyConstraintViolations, ngskit4b/KAligner.cpp:2716-2765)
and chromosome filters (`-Z` / `-z <regex>`, CKAligner::FiltByChroms :4025-4091) from the REAL reference front end
(`oracle/_ref/ngskit4b`, built by `make -C oracle ngskit4b`), run with ONE thread.

    python tests/golden/make_golden_filter.py

Per case (filter_cases.json): the kalign arguments -- `loci` names the constraints fixture given as -5, `exclude` / `include` are the
-Z / -z expressions (k4align takes them as --chromexclude / --chromeinclude) --, what the reference wrote (filter_<case>.sam.xz / .bam,
the SNP CSV of -p5, the three files of -O) and its NAR histogram.  For the restatement in tests/filter_ref.py: the names of the reads
the reference marked LC / FC / DP in the same run under -M1 (filter_marks.json.xz), and the -M1 SAM of the run without -5 / -Z / -z /
-k / -p / -O (filter_base_*.sam.xz, one per distinct command line).  The read sets are those of the pcrdup and stats goldens; the
constraint files (filter_lc_*.csv) are a few lines each.  Data only.
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

# the constraint files.  g1: chr1 60000, chr2 40000, chr3 25000, chr4 300, chr5 120 bp; g3: chr1 40000, chr2 30000, chr3 20000 bp
CSV = {
    # a title line; R, a letter set, a single locus, two constraints over one stretch (chr1 5000-6000 lies inside 1000-30000)
    "filter_lc_a.csv": '"Chrom","Start","End","Bases"\nchr1,1000,30000,R\nchr2,500,20000,ACG\nchr3,100,100,RT\nchr1,5000,6000,AC\n',
    # no title line, out of order, a quoted name, lower case and blanks in the bases, a comment, a blank line; the last locus of chr4
    "filter_lc_b.csv": 'chr2,500,20000,a c g\n# the same constraints as filter_lc_a.csv, and two more\n\n"chr1",1000,30000,r\nCHR3,100,100,tr\n'
                       "chr1,5000,6000,CA\nchr4,299,299,R\nchr1,0,0,ACGT\n",
    # the three lines of the issue's trial run
    "filter_lc_3.csv": "chr1,1000,30000,R\nchr2,500,20000,ACG\nchr3,100,100,RT\n",
    # for the g3 sets (flank-trimmed and two-segment reads)
    "filter_lc_g3.csv": "chr1,0,39999,R\nchr2,1000,25000,ACG\nchr3,500,15000,RT\nchr3,600,700,AG\n",
}

# name: (reads (-i[, -u]), index, kalign args, loci fixture, exclude, include, output extension)
CASES = {
    "excl": (["pcrdup_a.fa.xz"], "g1", ["-s2"], None, ["chr[45]"], [], "sam"),
    "incl_excl": (["pcrdup_a.fa.xz"], "g1", ["-s2"], None, ["chr2"], ["chr[12]$"], "sam"),
    "incl_none": (["pcrdup_a.fa.xz"], "g1", ["-s2"], None, [], ["^nosuch"], "sam"),
    "excl_two_M1": (["pcrdup_a.fa.xz"], "g1", ["-s2", "-M1"], None, ["chr4", "^chr5$"], ["chr"], "sam"),
    "lc_a": (["pcrdup_a.fa.xz"], "g1", ["-s2"], "filter_lc_a.csv", [], [], "sam"),
    "lc_b_M1": (["pcrdup_a.fa.xz"], "g1", ["-s2", "-M1"], "filter_lc_b.csv", [], [], "sam"),
    "lc_k20_excl_M1": (["pcrdup_a.fa.xz"], "g1", ["-s2", "-M1", "-k20"], "filter_lc_3.csv", ["chr4"], [], "sam"),
    "lc_x5_excl": (["pcrdup_a.fa.xz"], "g1", ["-s3", "-x5"], "filter_lc_a.csv", ["chr3"], [], "sam"),
    "lc_c50": (["pcrdup_c.fa.xz"], "g3", ["-s2", "-c50"], "filter_lc_g3.csv", [], [], "sam"),
    "lc_gap_a12_A3000": (["stats_gap.fa.xz"], "g1", ["-s2", "-a12", "-A3000"], "filter_lc_a.csv", [], [], "sam"),
    "lc_seg_a12_A3000": (["sam_se_all_120.fa.xz"], "g3", ["-s2", "-a12", "-A3000"], "filter_lc_g3.csv", ["chr3"], [], "sam"),
    "lc_pe_u1": (["pcrdup_p_1.fa.xz", "pcrdup_p_2.fa.xz"], "g1", ["-s2", "-U1", "-d200", "-D600"], "filter_lc_3.csv", [], [], "sam"),
    "lc_pe_u3_M1": (["pcrdup_p_1.fa.xz", "pcrdup_p_2.fa.xz"], "g1", ["-s2", "-U3", "-d200", "-D600", "-M1"], "filter_lc_a.csv", [], [], "sam"),
    "lc_excl_bam": (["pcrdup_a.fa.xz"], "g1", ["-s2"], "filter_lc_a.csv", ["chr[45]"], [], "bam"),
    "lc_excl_p5": (["pcrdup_a.fa.xz"], "g1", ["-s2", "-p5"], "filter_lc_3.csv", ["chr3"], [], "sam"),
    "lc_excl_O": (["pcrdup_a.fa.xz"], "g1", ["-s2", "-O"], "filter_lc_a.csv", ["chr2"], [], "sam"),
    "excl_j": (["pcrdup_a.fa.xz"], "g1", ["-s2", "-j"], "filter_lc_3.csv", ["chr[45]"], [], "sam"),
}
STRIP_BASE = ("-k", "-p", "-O", "-M", "-j")  # the base run: none of the filters, none of what reports; -x and the orphan filters stay


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


def kalign(sfx, out, args, files, loci=None, excl=(), incl=()):
    cmd = [NGS, "kalign", "-I", sfx, "-o", out, "-T", "1", "-F", out + ".log"]
    for a in args:  # -O / -j take a file beside the output
        cmd += [a, out + (".stats.csv" if a == "-O" else ".none.fa")] if a in ("-O", "-j") else [a]
    if loci:
        cmd += ["-5", os.path.join(HERE, loci)]
    for e in excl:
        cmd += ["-Z", e]
    for e in incl:
        cmd += ["-z", e]
    subprocess.run(cmd + files, check=True, capture_output=True, timeout=900)
    return hist_of(out + ".log")


def main():
    for name, text in CSV.items():
        with open(os.path.join(HERE, name), "w", newline="") as f:
            f.write(text)
    with tempfile.TemporaryDirectory() as tmp:
        sfx = {"g1": os.path.join(HERE, "g1.sfx"), "g3": unxz("g3.sfx.xz", os.path.join(tmp, "g3.sfx"))}
        meta, marks, bases = {}, {}, {}
        for name, (reads, index, args, loci, excl, incl, ext) in CASES.items():
            files = []
            for flag, r in zip(("-i", "-u"), reads):
                files += [flag, unxz(r, os.path.join(tmp, r[:-3]))]
            out = os.path.join(tmp, "%s.%s" % (name, ext))
            hist = kalign(sfx[index], out, args, files, loci, excl, incl)
            m = dict(reads=reads, index=index, args=args, loci=loci, exclude=excl, include=incl, out=ext, nar=hist, files=[])
            if ext == "bam":
                shutil.copy(out, os.path.join(HERE, "filter_%s.bam" % name))
            else:
                xz(out, "filter_%s.sam.xz" % name)
            if "-p5" in args:
                xz(out + ".snp", "filter_%s.snp.xz" % name)  # (kalign -p without -S: <out>.snp)
            if "-j" in args:
                xz(out + ".none.fa", "filter_%s.none.xz" % name)
            if "-O" in args:
                for key, path in (("main", out + ".stats.csv"), ("cnts", out + ".stats.AlignCntsDist.csv")):
                    xz(path, "filter_%s.%s.xz" % (name, key))
                    m["files"].append(key)
            # the reads the reference marked: the same run as -M1, the reports left out (kalign refuses -M1 with SNP calling)
            m1 = out
            if "-M1" not in args:
                m1 = os.path.join(tmp, name + ".m1.sam")
                kalign(sfx[index], m1, [a for a in args if not a.startswith(("-p", "-M", "-O", "-j"))] + ["-M1"], files, loci, excl, incl)
            marks[name] = {code: sorted(l.split("\t", 2)[0] + "/" + str((int(l.split("\t", 2)[1]) >> 7) & 1) for l in open(m1) if l.endswith("YU:Z:%s\n" % code))
                           for code in ("LC", "FC", "DP")}
            # the run without the filters, every loaded read reported: one file per distinct command line
            bargs = [a for a in args if not a.startswith(STRIP_BASE)] + ["-M1"]
            bname = "filter_base_%s_%s.sam.xz" % (reads[0].split(".")[0], "_".join(a.lstrip("-") for a in bargs))
            if bname not in bases:
                base = os.path.join(tmp, name + ".base.sam")
                bases[bname] = kalign(sfx[index], base, bargs, files)
                xz(base, bname)
            m["base"], m["base_nar"] = bname, bases[bname]
            meta[name] = m
            print(name, {k: v for k, v in hist.items() if v}, {k: len(v) for k, v in marks[name].items()})
        # ---- the cases exercise what they are there for ---------------------------------------------------------------------------
        assert meta["incl_none"]["nar"]["AA"] == 0 and meta["incl_none"]["nar"]["FC"] == meta["incl_none"]["base_nar"]["AA"]
        for name, m in meta.items():
            if m["loci"]:
                assert m["nar"]["LC"] > 0, name
            if m["exclude"] or m["include"]:
                assert m["nar"]["FC"] > 0, name
            assert m["nar"]["LC"] == len(marks[name]["LC"]) and m["nar"]["FC"] == len(marks[name]["FC"]), name
        assert meta["lc_k20_excl_M1"]["nar"]["DP"] > 100
        with open(os.path.join(HERE, "filter_cases.json"), "w") as f:  # one case per line
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(meta.items())) + "\n}\n")
        with lzma.open(os.path.join(HERE, "filter_marks.json.xz"), "wt", preset=9) as f:
            json.dump(marks, f, sort_keys=True)


if __name__ == "__main__":
    main()
