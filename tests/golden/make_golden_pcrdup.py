"""Golden outputs of kalign's PCR artefact reduction (`-k <WinLen>`, CKAligner::ReducePCRduplicates, ngskit4b/KAligner.cpp:2303-2400)
from the REAL reference front end (`oracle/_ref/ngskit4b`, built by `make -C oracle ngskit4b`), run with ONE thread so that reads
with equal SortHitMatch keys keep their load order.

    python tests/golden/make_golden_pcrdup.py

Per case (pcrdup_cases.json): the command line, what the reference wrote (SAM / BAM / SNP CSV) and its NAR histogram; for SE the
names of the reads it marked DP (pcrdup_dp_names.json.xz, from the same run with -M1) and the SAM of the run without -k and without
the stages that run after it, -x and -p (pcrdup_base_*.sam.xz, one per distinct command line) -- the input of the restatement in
tests/pcrdup_ref.py.  The reads (pcrdup_<set>.fa.xz) hold stacks of 2 to a few hundred
copies of one fragment (some copies with substitutions), tilings dense enough to reach every LimitDups bucket, stacks on both strands
at one start, equal starts with different lengths, stacks near chromosome starts, and (set c) reads with foreign flanks for -c.
Data only.
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


def stack_reads(chroms, seed, n_stacks=70, n_tiles=8, chimeric=0.0):
    """duplicate stacks, dense tilings and background reads over `chroms` (lists of etSeqBase codes)"""
    rng = np.random.default_rng(seed)
    reads = []
    lens = [len(c) for c in chroms]

    def frag(c, start, L, strand, subs, flank=False):
        rd = chroms[c][start:start + L].copy()
        for p in rng.choice(L, size=subs, replace=False) if subs else ():
            rd[p] = (rd[p] + int(rng.integers(1, 4))) % 4
        if flank:  # foreign sequence at one or both ends: -c trims it off (a soft clip)
            for side in (0, 1):
                if rng.random() < 0.6:
                    k = int(rng.integers(L * 8 // 100, L * 30 // 100))
                    if side == 0:
                        rd[:k] = rng.integers(0, 4, k)
                    else:
                        rd[L - k:] = rng.integers(0, 4, k)
        return synth.revcomp(rd) if strand else rd

    def copies():  # 2 .. a few hundred, mostly small
        u = rng.random()
        return int(rng.integers(2, 6)) if u < 0.55 else int(rng.integers(6, 30)) if u < 0.85 else int(rng.integers(30, 120)) if u < 0.96 else int(rng.integers(150, 320))

    for s in range(n_stacks):
        c = int(rng.integers(0, len(chroms)))
        L = int(rng.choice([60, 80, 100]))
        if lens[c] < L + 2:
            continue
        near_start = rng.random() < 0.15
        start = int(rng.integers(0, min(250, lens[c] - L))) if near_start else int(rng.integers(0, lens[c] - L))
        strands = [0, 1] if rng.random() < 0.25 else [int(rng.integers(0, 2))]
        for strand in strands:
            Ls = [L] if rng.random() < 0.7 else sorted({L, int(rng.choice([60, 80, 100]))})  # equal starts, different lengths
            for LL in Ls:
                if start + LL > lens[c]:
                    continue
                for k in range(copies()):
                    subs = 0 if rng.random() < 0.6 else int(rng.integers(1, 3))
                    reads.append(frag(c, start, LL, strand, subs, flank=chimeric > 0 and rng.random() < chimeric))
    # tilings: a start every `step` bases over a region, each site stacked 1..6 deep -- the window counts of every bucket
    for t in range(n_tiles):
        step = [1, 1, 2, 3, 5, 8, 13, 25][t % 8]
        c = int(rng.integers(0, min(3, len(chroms))))
        span = int(rng.integers(300, 700))
        L = 80
        base = 0 if t % 4 == 0 else int(rng.integers(0, lens[c] - span - L))  # some tilings from the chromosome's first base
        strand = int(rng.integers(0, 2))
        for p in range(base, base + span, step):
            for k in range(int(rng.integers(1, 7))):
                reads.append(frag(c, p, L, strand if rng.random() < 0.8 else 1 - strand, 0 if rng.random() < 0.7 else 1))
    # background: unique reads, unalignable reads
    reads += synth.make_reads(chroms, 800, 100, seed=seed + 1, sub_lambda=1.0, edge_frac=0.05, random_frac=0.05)[0]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def g3_genome():
    from make_golden_ext import genome

    names, chroms, _, _ = genome()
    return names, chroms


# name: (read set, index, kalign args, output extension)
CASES = {
    "k0": ("a", "g1", ["-s2", "-k0"], "sam"),
    "k5": ("a", "g1", ["-s2", "-k5"], "sam"),
    "k50": ("a", "g1", ["-s2", "-k50"], "sam"),
    "k250": ("a", "g1", ["-s2", "-k250"], "sam"),
    "k20_x5": ("a", "g1", ["-s3", "-k20", "-x5"], "sam"),
    "k20_r3_R8": ("a", "g1", ["-s2", "-k20", "-r3", "-R8"], "sam"),
    "k20_M1": ("a", "g1", ["-s2", "-k20", "-M1"], "sam"),
    "k20_bam": ("a", "g1", ["-s2", "-k20"], "bam"),
    "k20_p5": ("a", "g1", ["-s2", "-k20", "-p5"], "sam"),
    "k20_c50": ("c", "g3", ["-s2", "-k20", "-c50"], "sam"),
    "pe_u1_k20": ("p", "g1", ["-s2", "-U1", "-d200", "-D600", "-k20"], "sam"),
}
STRIP_BASE = ("-k", "-x", "-p", "-M")  # the base run: no -k and none of what runs behind it


def hist_of(log):
    hist = {}
    for line in open(log):
        m = re.search(r"\)\s+(\d+) \((\w\w)\) ", line)
        if m:
            hist[m.group(2)] = int(m.group(1))
    return hist


def kalign(tmp, sfx, out, args, files):
    log = out + ".log"
    subprocess.run([NGS, "kalign", "-I", sfx, "-o", out, "-T", "1", "-F", log] + args + files, check=True, capture_output=True, timeout=900)
    return hist_of(log)


def xz(src, dst):
    with open(src, "rb") as f, lzma.open(os.path.join(HERE, dst), "wb", preset=9) as g:
        g.write(f.read())


def main():
    _, g1 = synth.golden_genome()
    with tempfile.TemporaryDirectory() as tmp:
        g3sfx = os.path.join(tmp, "g3.sfx")
        with lzma.open(os.path.join(HERE, "g3.sfx.xz")) as f, open(g3sfx, "wb") as g:
            shutil.copyfileobj(f, g)
        sfx = {"g1": os.path.join(HERE, "g1.sfx"), "g3": g3sfx}
        sets = {}
        ra = stack_reads(g1, 0x9C01)
        sets["a"] = [("-i", "pcrdup_a.fa", ra)]
        rc = stack_reads(g3_genome()[1], 0x9C02, n_stacks=50, n_tiles=4, chimeric=0.4)
        sets["c"] = [("-i", "pcrdup_c.fa", rc)]
        pe1, pe2, _ = synth.make_pe_reads(g1, 1500, 100, seed=0x9C03, sub_lambda=1.0)
        dup1, dup2 = [], []
        rng = np.random.default_rng(0x9C04)
        for i in rng.choice(len(pe1), 150, replace=False):  # duplicated pairs: PE ignores -k
            for k in range(int(rng.integers(2, 12))):
                dup1.append(pe1[i].copy())
                dup2.append(pe2[i].copy())
        sets["p"] = [("-i", "pcrdup_p_1.fa", pe1 + dup1), ("-u", "pcrdup_p_2.fa", pe2 + dup2)]
        files = {}
        for key, lst in sets.items():
            files[key] = []
            for flag, name, reads in lst:
                path = os.path.join(tmp, name)
                synth.write_fasta(path, reads)
                xz(path, name + ".xz")
                files[key] += [flag, path]
        meta, dp_names, bases = {}, {}, {}
        for name, (rs, index, args, ext) in CASES.items():
            out = os.path.join(tmp, "%s.%s" % (name, ext))
            hist = kalign(tmp, sfx[index], out, args, files[rs])
            m = dict(reads=rs, index=index, args=args, out=ext, nar=hist)
            if ext == "bam":
                shutil.copy(out, os.path.join(HERE, "pcrdup_%s.bam" % name))
            else:
                xz(out, "pcrdup_%s.sam.xz" % name)
            if "-p5" in args:
                xz(out + ".snp", "pcrdup_%s.snp.xz" % name)  # (kalign -p without -S: <out>.snp)
            meta[name] = m
            if rs == "p":  # (PE: -k does nothing; the test compares with the run without it)
                continue
            # the reads marked DP: the same run as -M1 (YU:Z:DP), SNP calling left out (kalign refuses -M1 with it)
            m1 = out
            if "-M1" not in args:
                m1 = os.path.join(tmp, name + ".m1.sam")
                kalign(tmp, sfx[index], m1, [a for a in args if not a.startswith(("-p", "-M"))] + ["-M1"], files[rs])
            dp_names[name] = sorted(l.split("\t", 1)[0] for l in open(m1) if l.endswith("YU:Z:DP\n"))
            # the run without -k: one file per distinct command line
            bargs = [a for a in args if not a.startswith(STRIP_BASE)]
            bname = "pcrdup_base_%s_%s.sam.xz" % (rs, "_".join(a.lstrip("-") for a in bargs))
            if bname not in bases:
                base = os.path.join(tmp, name + ".base.sam")
                bases[bname] = kalign(tmp, sfx[index], base, bargs, files[rs])
                xz(base, bname)
            m["base"], m["base_nar"] = bname, bases[bname]
            print(name, hist.get("AA"), hist.get("DP"), len(dp_names[name]))
        with open(os.path.join(HERE, "pcrdup_cases.json"), "w") as f:  # one case per line
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(meta.items())) + "\n}\n")
        with lzma.open(os.path.join(HERE, "pcrdup_dp_names.json.xz"), "wt", preset=9) as f:
            json.dump(dp_names, f, sort_keys=True)

if __name__ == "__main__":
    main()
