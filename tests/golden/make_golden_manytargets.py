"""Golden data on the 300-target genome of tests/manytargets.py, from the REAL reference (needs `make -C oracle ref ngskit4b`):

    python tests/golden/make_golden_manytargets.py [npz] [sam]

npz  align_mt300_*.npz, in the format of make_golden.py's align_*.npz: what the reference's CSfxArray::AlignReads returned on the
     index the oracle's builder wrote for manytargets.genome(300).  (Byte-identical targets make suffixes that tie through their
     EOS; the reference's own builder leaves those in an unspecified order, the oracle's orders them by offset, and the order
     decides the order of a read's hit records.  A test rebuilds this index with the oracle and needs no reference.)
sam  mt300_<case>*.fa.xz, mt300_<case>.sam.xz and mt300_cases.json: the FASTA of the genome goes through `ngskit4b index`, the
     reads through `ngskit4b kalign`; the JSON records the command lines, the NAR tallies and the SHA-256 of the reference's
     .sfx and of its parts (the file is not kept: `k4index` has to write the same one).

Data only.
"""
import hashlib
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
import manytargets  # noqa: E402
import synth  # noqa: E402
from oracle_bindings import HIT_DTYPE, Oracle, Ref, flatten_reads  # noqa: E402

NGS = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")

# (name, read_len, TotMM, CoreLen, CoreDelta, MaxNumCoreSlides, MaxHits, MMDelta, strand, MaxIter, reads of make_reads, seed)
NPZ_CASES = [  # (the names: manytargets.NPZ_CASES)
    ("mt300_se_s2", 100, 2, 33, 33, 8, 1, 1, 0, 5000, 2800, 3001),
    ("mt300_s3_150_mh10", 150, 3, 37, 37, 12, 10, 1, 0, 5000, 2400, 3002),
]


def _se_reads(chroms, n, seed, rl=100):
    return manytargets.raw_batch(chroms, n, rl, seed)[0]


def _pe_reads(chroms, seed):
    pe1, pe2, _, _ = manytargets.pe_batch(chroms, 1500, read_len=100, seed=seed, frag_min=220, frag_max=420)
    return pe1, pe2


# name: (kalign arguments, reads)
SAM_CASES = {
    "se_s2": (["-s2"], lambda ch: _se_reads(ch, 2600, 3101)),
    "se_s2_sq100": (["-s2", "-4", "100"], lambda ch: _se_reads(ch, 2600, 3101)),
    "se_r5_R8": (["-s2", "-r5", "-R8"], lambda ch: _se_reads(ch, 2600, 3102)),
    "pe_u2": (["-s2", "-U2", "-d200", "-D600"], lambda ch: _pe_reads(ch, 3103)),
    "pe_u2_sq100": (["-s2", "-U2", "-d200", "-D600", "-4", "100"], lambda ch: _pe_reads(ch, 3103)),
    "se_s2_M1": (["-s2", "-M1"], lambda ch: _se_reads(ch, 2600, 3101)),
}
SAME_READS = {"se_s2_sq100": "se_s2", "se_s2_M1": "se_s2", "pe_u2_sq100": "pe_u2"}  # cases that reuse another case's read files


def valid_hits(res, max_hits):
    h = res["hits"].copy()
    for i in range(len(h)):
        nh = min(int(res["inst"][i]), max_hits) if res["rslt"][i] in (1, 2, 3) else 0
        h[i, nh:] = np.zeros((), dtype=HIT_DTYPE)
    return h


def make_npz(tmp):
    O, R = Oracle(), Ref()
    names, chroms = manytargets.genome(300)
    sfx = os.path.join(tmp, "mt300_oracle.sfx")
    ho = O.build(names, chroms, dataset="mt300", threads=4)
    O.write(ho, sfx)
    O.close(ho)
    for (name, rl, tm, cl, cd, sl, mh, md, strand, maxiter, nreads, seed) in NPZ_CASES:
        hr = R.open(sfx, maxiter, 0)
        reads, _ = manytargets.raw_batch(chroms, nreads, rl, seed)
        res = R.align_reads_batch(hr, reads, tm, cl, cd, sl, 0, md, strand, mh)
        R.close(hr)
        cat, offs, lens = flatten_reads(reads)
        np.savez_compressed(os.path.join(HERE, "align_%s.npz" % name), reads=cat, offs=offs, lens=lens,
                            params=np.array([tm, cl, cd, sl, 0, md, strand, mh, maxiter], dtype=np.int32),
                            rslt=res["rslt"], inst=res["inst"], low=res["low"], nxt=res["nxt"], hits=valid_hits(res, mh))
        acc = res["rslt"] == 1
        print(name, "rslt hist", np.bincount(res["rslt"], minlength=5), "max inst", res["inst"].max(), "accepted on id > 128:",
              int((res["hits"][acc, 0]["chrom_id"] > 128).sum()))


def _xz(src, dst):
    with open(src, "rb") as f, lzma.open(dst, "wb", preset=9) as g:
        g.write(f.read())


def make_sam(tmp):
    names, chroms = manytargets.genome(300)
    fa = os.path.join(tmp, "mt300.fa")
    synth.write_fasta(fa, chroms, names=names)
    sfx = os.path.join(tmp, "mt300.sfx")
    subprocess.run([NGS, "index", "-i", fa, "-o", sfx, "-r", "mt300", "-T", "4", "-F", os.path.join(tmp, "index.log")], check=True,
                   capture_output=True)
    raw = open(sfx, "rb").read()
    meta = {"sfx_sha256": hashlib.sha256(raw).hexdigest(), "sfx_bytes": len(raw), "sfx_parts_sha256": manytargets.sfx_parts(raw), "cases": {}}
    for name, (args, gen) in SAM_CASES.items():
        base = SAME_READS.get(name, name)
        files, stored = [], []
        got = gen(chroms)
        for flag, suffix, reads in ((("-i", "_1", got[0]), ("-u", "_2", got[1])) if name.startswith("pe_") else (("-i", "", got),)):
            p = os.path.join(tmp, "%s%s.fa" % (base, suffix))
            if not os.path.exists(p):
                synth.write_fasta(p, reads)
                _xz(p, os.path.join(HERE, "mt300_%s%s.fa.xz" % (base, suffix)))
            files += [flag, p]
            stored.append("mt300_%s%s.fa.xz" % (base, suffix))
        sam, log = os.path.join(tmp, name + ".sam"), os.path.join(tmp, name + ".log")
        subprocess.run([NGS, "kalign", "-I", sfx, "-o", sam, "-T", "4", "-F", log] + args + files, check=True, capture_output=True,
                       timeout=600)
        hist = {}
        for line in open(log):
            m = re.search(r"\)\s+(\d+) \((\w\w)\) ", line)
            if m:
                hist[m.group(2)] = int(m.group(1))
        _xz(sam, os.path.join(HERE, "mt300_%s.sam.xz" % name))
        n_sq = sum(1 for l in open(sam) if l.startswith("@SQ"))
        meta["cases"][name] = dict(args=args, reads=stored, nar=hist, n_sq=n_sq)
        print(name, hist, "@SQ lines", n_sq)
    json.dump(meta, open(os.path.join(HERE, "mt300_cases.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    what = [a for a in sys.argv[1:]] or ["npz", "sam"]
    with tempfile.TemporaryDirectory() as tmp:
        if "npz" in what:
            make_npz(tmp)
        if "sam" in what:
            make_sam(tmp)
