"""Golden outputs of kalign's start-site octamer preferences (`-8 <file>`, `-9 <ofs>`: CKAligner::ProcessSiteProbabilites /
WriteSitePrefs, ngskit4b/KAligner.cpp:8708-8945) from the REAL reference front end (`oracle/_ref/ngskit4b`, built by
`make -C oracle ngskit4b`), run with ONE thread.

    python tests/golden/make_golden_siteprefs.py

Per case (siteprefs_cases.json): the command line, the reads, the NAR histogram of the reference's log, and what it wrote: the SAM
(siteprefs_<case>.sam.xz) and the site file (siteprefs_<case>.csv.xz).  The read sets are made here: duplicate stacks of distinct
depths on more than 64 sites per strand over a background of single reads, so that the 64 largest NumOccs / NumSites ratios are told
apart from the rest whatever order the reference's unstable sort leaves tied entries in.

Two conditions are checked from the reference's own output, and a case that breaks one is not written (the seed of its read set is
stepped until both hold):
  1. per strand the top-64 boundary is untied (siteprefs_ref.boundary_untied over the TotalHits / UniqueLoci columns);
  2. no accepted read has its signed octamer locus in -8..-1, where the reference reads an uninitialised array.
The script also checks that the cases exercise what they are there for.  Data only.
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
import siteprefs_ref  # noqa: E402
import synth  # noqa: E402

NGS = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")

# name: (index, read set made here (None: an existing file), kalign args)
CASES = {
    "se_default": ("g1", "a", ["-s2"]),
    "se_ofs0": ("g1", "a", ["-s2", "-9", "0"]),
    "se_ofs10": ("g1", "a", ["-s2", "-9", "10"]),
    "se_ofs_m100": ("g1", "a", ["-s2", "-9", "-100"]),
    "se_x5": ("g1", "a", ["-s3", "-x5"]),
    "se_k20": ("g1", "k", ["-s2", "-k20"]),
    "se_c50": ("g3", "c", ["-s2", "-c50"]),
    "se_a12_A3000": ("g3", "c", ["-s2", "-a12", "-A3000"]),
    "se_r3_R8": ("g2", "r", ["-s2", "-r3", "-R8"]),
    "pe_u1": ("g1", "p", ["-s2", "-U1", "-d200", "-D600"]),
    "se_nrun": ("g1", "n", ["-s2"]),
    "se_none": ("g1", None, ["-s2"]),
}
SETS = {"a": "g1", "k": "g1", "c": "g3", "r": "g2", "p": "g1", "n": "g1"}
FILES = {"a": ["siteprefs_a.fa"], "k": ["siteprefs_k.fa"], "c": ["siteprefs_c.fa"], "r": ["siteprefs_r.fa"], "p": ["siteprefs_p_1.fa", "siteprefs_p_2.fa"],
         "n": ["siteprefs_n.fa"], None: ["stats_none.fa"]}


def genomes():
    from make_golden_ext import genome

    g3 = genome()
    return {"g1": synth.golden_genome(), "g2": synth.cluster_genome()[:2], "g3": g3[:2]}, g3[2]


def ofs_of(args):
    return int(args[args.index("-9") + 1]) if "-9" in args else -4


def mutate(rng, rd, subs):
    for p in rng.choice(len(rd), size=subs, replace=False) if subs else ():
        if rd[p] <= 3:
            rd[p] = (rd[p] + int(rng.integers(1, 4))) % 4
    return rd


def stack_sites(rng, chroms, n_per_strand, L):
    """(chrom, start, strand, depth): depths 2, 3, 4, ... per strand, sites away from the sequence ends and from N"""
    sites = []
    for strand in (0, 1):
        depth = 2
        while depth < 2 + n_per_strand:
            c = int(rng.integers(0, len(chroms)))
            if len(chroms[c]) < L + 400:
                continue
            start = int(rng.integers(150, len(chroms[c]) - L - 150))
            if (chroms[c][start - 120:start + L + 120] > 3).any():
                continue
            sites.append((c, start, strand, depth))
            depth += 1
    return sites


def se_reads(chroms, seed, L=100, n_per_strand=84, background=1500, flank=0.0, extra=(), lengths=False):
    """lengths: -k keeps the first reads of every (start, length, strand): a site of depth d gets d - 1 read lengths, three reads of
    each, around one 5' end, so that the sites still differ in depth behind the reduction"""
    rng = np.random.default_rng(seed)
    reads = []
    for c, start, strand, depth in stack_sites(rng, chroms, n_per_strand, L):
        if lengths:
            for q in range(depth - 1):
                ln = 60 + q
                a = start + L - ln if strand else start
                for _ in range(3):
                    rd = chroms[c][a:a + ln].copy()
                    reads.append(synth.revcomp(rd) if strand else rd)
            continue
        for _ in range(depth):
            rd = mutate(rng, chroms[c][start:start + L].copy(), 0 if rng.random() < 0.6 else 1)
            if flank and rng.random() < flank:  # foreign sequence at an end: -c trims it off (a soft clip)
                k = int(rng.integers(8, 30))
                if rng.random() < 0.5:
                    rd[:k] = rng.integers(0, 4, k)
                else:
                    rd[L - k:] = rng.integers(0, 4, k)
            reads.append(synth.revcomp(rd) if strand else rd)
    bg, truth = synth.make_reads(chroms, background, L, seed=seed + 1, sub_lambda=1.0, edge_frac=0.08, random_frac=0.03)
    for rd, t in zip(bg, truth):  # (a Watson read within the first bases of a sequence is looked at by check 2 all the same)
        if not (t[2] == 0 and (t[1] < 4 or 92 <= t[1] < 100)):
            reads.append(rd)
    reads += list(extra)
    return [reads[i] for i in rng.permutation(len(reads))]


def pe_reads(chroms, seed, L=100, n_per_strand=84, background=900):
    rng = np.random.default_rng(seed)
    p1, p2 = [], []
    big = [c for c in chroms if len(c) > 5000]
    for c, start, strand, depth in stack_sites(rng, big, n_per_strand, 400):
        flen = int(rng.integers(300, 400))
        frag = big[c][start:start + flen]
        frag = synth.revcomp(frag) if strand else frag
        for _ in range(depth):
            p1.append(mutate(rng, frag[:L].copy(), 0 if rng.random() < 0.7 else 1))
            p2.append(mutate(rng, synth.revcomp(frag[flen - L:]), 0 if rng.random() < 0.7 else 1))
    a, b, truth = synth.make_pe_reads(big, background, L, seed=seed + 1)
    for x, y, t in zip(a, b, truth):
        if t[1] >= 100:
            p1.append(x)
            p2.append(y)
    order = rng.permutation(len(p1))
    return [p1[i] for i in order], [p2[i] for i in order]


def n_run_reads(chroms, seed, L=100):
    """reads whose octamer at the default offset (four bases in front of the read's 5' end) reaches into a run of N"""
    rng = np.random.default_rng(seed)
    reads = []
    for c, g in enumerate(chroms):
        isn = np.flatnonzero(g > 3)
        if not len(isn):
            continue
        runs = np.split(isn, np.flatnonzero(np.diff(isn) > 1) + 1)
        for run in runs:
            a, b = int(run[0]), int(run[-1]) + 1  # [a, b) is N
            for d in range(0, 8):
                if b + d + L <= len(g) and not (g[b + d:b + d + L] > 3).any():
                    reads.append(g[b + d:b + d + L].copy())  # Watson, starting d bases behind the run
                if a - d - L >= 0 and not (g[a - d - L:a - d] > 3).any():
                    reads.append(synth.revcomp(g[a - d - L:a - d]))  # Crick, its 5' end d bases in front of the run
    assert len(reads) > 20
    return [mutate(rng, r, 0 if rng.random() < 0.7 else 1) for r in reads]


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


def columns(site_text):
    """NumOccs, NumSites [2, 65536] of a site file (the row of tttttttt is not in it: zero here)"""
    occ, sites = np.zeros((2, 65536), np.int64), np.zeros((2, 65536), np.int64)
    for line in site_text.splitlines()[1:]:
        f = line.split(",")
        s = 0 if f[1] == '"+"' else 1
        occ[s, int(f[0]) - 1], sites[s, int(f[0]) - 1] = int(f[3]), int(f[4])
    return occ, sites


def signed_loci(r, ofs):
    return r["loci"] + ofs if r["strand"] == "+" else r["loci"] + r["mlen"] - 1 - ofs - 7


def run_case(tmp, sfx, name, files, args):
    out, site, log = os.path.join(tmp, name + ".sam"), os.path.join(tmp, name + ".site.csv"), os.path.join(tmp, name + ".log")
    fl = []
    for flag, f in zip(("-i", "-u"), files):
        fl += [flag, f]
    subprocess.run([NGS, "kalign", "-I", sfx, "-o", out, "-8", site, "-T", "1", "-F", log] + args + fl, check=True, capture_output=True, timeout=900)
    return open(out).read(), open(site).read(), hist_of(log)


def checks(name, sam, site, names, args):
    """the two conditions; returns the accepted records"""
    recs = siteprefs_ref.records_of_sam(sam, names)
    if not site:
        return recs, True
    occ, sites = columns(site)
    ok = all(siteprefs_ref.boundary_untied(occ[s], sites[s]) for s in (0, 1))
    ok &= not any(-8 <= signed_loci(r, ofs_of(args)) <= -1 for r in recs if not r["segs"])
    return recs, ok


def main():
    gen, splice_sites = genomes()
    with tempfile.TemporaryDirectory() as tmp:
        sfx = {"g1": os.path.join(HERE, "g1.sfx"), "g2": unxz("g2.sfx.xz", os.path.join(tmp, "g2.sfx")),
               "g3": unxz("g3.sfx.xz", os.path.join(tmp, "g3.sfx"))}
        unxz("stats_none.fa.xz", os.path.join(tmp, "stats_none.fa"))
        results = {}
        for key, index in SETS.items():
            chroms = gen[index][1]
            mine = [c for c in CASES if CASES[c][1] == key]
            for attempt in range(12):
                seed = 0x5170 + 0x100 * (ord(key) - ord("a")) + attempt
                if key == "p":
                    sets = pe_reads(chroms, seed)
                elif key == "n":
                    sets = [se_reads(chroms, seed, extra=n_run_reads(chroms, seed + 7))]
                elif key == "c":
                    extra = synth.make_variant_reads(chroms, 12, 6, 100, "indel", seed=seed + 3) + \
                        synth.make_variant_reads(chroms, 12, 6, 100, "splice", seed=seed + 4, sites=splice_sites)
                    sets = [se_reads(chroms, seed, flank=0.3, extra=extra)]
                elif key == "k":
                    sets = [se_reads(chroms, seed, n_per_strand=72, lengths=True)]
                else:
                    sets = [se_reads(chroms, seed)]
                paths = [os.path.join(tmp, f) for f in FILES[key]]
                for p, s in zip(paths, sets):
                    synth.write_fasta(p, s)
                got, good = {}, True
                for c in mine:
                    sam, site, hist = run_case(tmp, sfx[index], c, paths, CASES[c][2])
                    recs, ok = checks(c, sam, site, gen[index][0], CASES[c][2])
                    got[c] = (sam, site, hist, recs)
                    good &= ok
                    if not ok:
                        print("set %s seed %#x: case %s breaks a condition" % (key, seed, c))
                        break
                if good:
                    break
            else:
                raise SystemExit("no seed of set %s passes" % key)
            print("set %s: seed %#x" % (key, seed))
            for p in paths:
                xz(p, os.path.basename(p) + ".xz")
            results.update(got)
        sam, site, hist = run_case(tmp, sfx["g1"], "se_none", [os.path.join(tmp, "stats_none.fa")], CASES["se_none"][2])
        results["se_none"] = (sam, site, hist, siteprefs_ref.records_of_sam(sam, gen["g1"][0]))
        # ---- the cases exercise what they are there for -------------------------------------------------------------------------
        assert results["se_none"][1] == "" and results["se_none"][2].get("AA") == 0
        assert any(signed_loci(r, -100) < -8 for r in results["se_ofs_m100"][3]), "no wrap-then-clamp read"
        for c in ("se_c50", "se_x5"):
            assert any(r["clipped"] and not r["segs"] for r in results[c][3]), c
        assert any(r["segs"] for r in results["se_a12_A3000"][3]), "no two-segment read"
        assert results["se_k20"][2].get("DP", 0) > 100
        chroms = gen["g1"][1]
        assert any(not r["segs"] and 0 <= signed_loci(r, -4) and (chroms[r["chrom"] - 1][signed_loci(r, -4):signed_loci(r, -4) + 8] > 3).any()
                   for r in results["se_nrun"][3]), "no octamer meets an N run"
        assert any(int(l.split("\t")[1]) & 1 for l in results["pe_u1"][0].splitlines() if not l.startswith("@"))
        meta = {}
        for c, (sam, site, hist, recs) in results.items():
            for text, ext in ((sam, "sam"), (site, "csv")):
                with lzma.open(os.path.join(HERE, "siteprefs_%s.%s.xz" % (c, ext)), "wt", preset=9) as f:
                    f.write(text)
            meta[c] = dict(index=CASES[c][0], reads=[f + ".xz" for f in FILES[CASES[c][1]]], args=CASES[c][2], nar=hist)
            print(c, hist.get("AA"), len(site))
        with open(os.path.join(HERE, "siteprefs_cases.json"), "w") as f:  # one case per line
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(meta.items())) + "\n}\n")


if __name__ == "__main__":
    main()
