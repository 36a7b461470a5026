"""Crafted inputs of the 5' primer correction stage (k4_pcr5_primer_correct_dev) over the genome behind tests/golden/g1.sfx: reads cut
from it at known loci with planted substitutions, as device-layout arrays, and the same records as the dicts tests/primer_ref.py
walks.  tests/test_primer_cpu.py checks that they make the claims they are meant to make; tests/test_gpu_primer.py runs them."""
import random

import numpy as np

import primer_ref

LENS = (50, 99, 100, 101, 150)  # around the rounding of (s * len + 50) / 100
RESULT_DTYPE = np.dtype([("hit_rslt", "<i4"), ("inst", "<i4"), ("low_mm", "<i4"), ("nxt_mm", "<i4"), ("nar", "<i4"), ("num_hits", "<i4")])
HIT_DTYPE = np.dtype([("chrom_id", "<u4"), ("match_loci", "<u4"), ("match_len", "<u2"), ("strand", "u1"), ("mismatches", "u1"), ("reserved", "<u4")])
PE_READ_DTYPE = np.dtype([("nar", "<i4"), ("num_hits", "<i4"), ("inst", "<i4"), ("low_mm", "<i4"), ("pe_aligned", "<i4"), ("rescued", "<i4"),
                          ("hit", HIT_DTYPE)])


def craft(chroms, n, seed):
    """n records.  Returns dict(reads, offs, lens, rr, hits) in the device layout and `recs`, the dicts of primer_ref (their seq: views
    are not shared with `reads`)."""
    rng = random.Random(seed)  # (scalar draws: far cheaper than numpy's one at a time)
    chroms = [np.asarray(c, np.uint8) for c in chroms]
    n_at = [np.flatnonzero(c == 4).tolist() for c in chroms]
    with_n = [k for k, a in enumerate(n_at) if len(a)]
    reads, recs = [], []
    rr = np.zeros(n, RESULT_DTYPE)
    hits = np.zeros(n, HIT_DTYPE)
    lens = np.zeros(n, np.uint32)
    for i in range(n):
        u = rng.random()
        c = rng.choice([3, 4]) if u < 0.10 else rng.choice(with_n) if u < 0.16 and with_n else rng.randrange(3)
        L = len(chroms[c])
        ln = rng.choice([x for x in LENS if x <= L])
        minus = bool(rng.random() < 0.5)
        v = rng.random()
        if u >= 0.10 and u < 0.16 and with_n:  # the 12 loci that face the read's first bases hold an N
            p = rng.choice(n_at[c]) + rng.randrange(-11, 1) * (-1 if minus else 1)
            loci = p - ln + 1 if minus else p
        elif v < 0.08:
            loci = 0            # '+': the read starts on locus 0 of the sequence; '-': its last bases face it
        elif v < 0.16:
            loci = L - ln       # '-': the read's first bases face the sequence's last loci
        else:
            loci = rng.randrange(L - ln + 1)
        loci = min(max(loci, 0), L - ln)
        targ = chroms[c][loci:loci + ln].tolist()
        if minus:
            targ = primer_ref.reverse_complement(targ)
        seq = list(targ)
        a, b = rng.randrange(5), rng.randrange(7)
        front = set(rng.sample(range(12), a))
        back = set(rng.sample(range(12, ln), b))
        w = rng.random()
        if w < 0.15 and a:
            front.pop(); front.add(11)
        elif w < 0.30 and b:
            back.pop(); back.add(12)
        for q in front | back:
            seq[q] = (targ[q] + rng.randrange(1, 4)) % 4 if targ[q] < 4 else rng.randrange(4)
        if rng.random() < 0.04:
            seq[rng.randrange(12)] = 4  # an N among the read's first 12
        mm = sum(1 for x, y in zip(seq, targ) if x != y)
        raw = [(hb & 0xF8) | s for hb, s in zip(rng.randbytes(ln), seq)]  # bits 3..7: what the stage has to keep
        nar = 1 if rng.random() >= 0.08 else rng.choice([0, 2, 3, 4, 5, 6, 9])
        x = rng.random()
        two = x < 0.03
        match_len = ln - rng.randrange(1, 6) if 0.03 <= x < 0.06 else ln
        rr[i] = (1, 1 if nar == 1 else 0, mm, mm + 1, nar, 1 if nar == 1 else 0)
        hits[i] = (c + 1, loci, match_len, ord("-" if minus else "+"), mm, ((1 << 25) if x < 0.015 else (1 << 27)) if two else 0)
        lens[i] = ln
        reads.append(np.array(raw, np.uint8))
        recs.append(dict(nar=nar, num_hits=int(rr[i]["num_hits"]), two_seg=two, match_len=match_len, loci=loci, chrom=c + 1,
                         strand="-" if minus else "+", read_len=ln, low_mm=mm, mismatches=mm, seq=list(raw), planted=(len(front), len(back)),
                         front=front, back=back))
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return dict(reads=np.concatenate(reads), offs=offs, lens=lens, rr=rr, hits=hits, recs=recs)


def expected(s, max_subs, chroms):
    """the arrays of `s` as the stage has to leave them under max_subs, the three totals, and per record the bases it rewrites"""
    recs = [dict(r, seq=list(r["seq"])) for r in s["recs"]]
    totals = primer_ref.pcr5_primer_correct(recs, max_subs, primer_ref.genome_target(chroms))
    rr, hits, reads = s["rr"].copy(), s["hits"].copy(), s["reads"].copy()
    fixed = np.zeros(len(recs), np.int64)
    for i, (r, r0) in enumerate(zip(recs, s["recs"])):
        rr[i]["nar"], rr[i]["num_hits"], rr[i]["low_mm"] = r["nar"], r["num_hits"], r["low_mm"]
        hits[i]["mismatches"] = r["mismatches"]
        if r["seq"] != r0["seq"]:
            o = int(s["offs"][i])
            reads[o:o + len(r["seq"])] = r["seq"]
            fixed[i] = sum(1 for x, y in zip(r["seq"], r0["seq"]) if x != y)
    return dict(rr=rr, hits=hits, reads=reads, totals=totals, fixed=fixed, recs=recs)


def as_pe(rr, hits):
    pe = np.zeros(len(rr), PE_READ_DTYPE)
    for k in ("nar", "num_hits", "inst", "low_mm"):
        pe[k] = rr[k]
    pe["pe_aligned"] = rr["nar"] == 1
    pe["hit"] = hits
    return pe
