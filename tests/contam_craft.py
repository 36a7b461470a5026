"""Crafted inputs for the tests of kalign's contaminant flank trimming (`-H`): the smallest shapes at which the packed compare of
k4_contam_rule.h, the host rule and the kernel of k4_contam.hip can go wrong.  A case is (contaminant FASTA text, trim5, trim3, PE1 read,
PE2 read or None, note); what a case must give comes from contam_ref, and `expect` pins the cases whose answer is plain by design.

Read lengths 19 (not examined), 20, 63, 64, 65, 199, 200, 201, 2000, 2001 (not examined); contaminant lengths 4, 31, 32, 33, 63, 64, 65,
200; substitutions at the first, last and word-boundary positions of an overlap; Ns on either side; the classes and the end trims."""
import numpy as np

import contam_ref as R

READ_LENS = [19, 20, 63, 64, 65, 199, 200, 201, 2000, 2001]
CONTAM_LENS = [4, 31, 32, 33, 63, 64, 65, 200]


def fasta(recs):
    return "".join(">%s\n%s\n" % (n, R.letters(s)) for n, s in recs).encode()


def _rand(rng, n):
    return [int(x) for x in rng.integers(0, 4, n)]


def _other(b):
    return (b + 1) % 4


def lengths_table(rng):
    """one contaminant per length, on every class as read (codes 1..4)"""
    return [("len%d@1234" % n, _rand(rng, n)) for n in CONTAM_LENS]


def cases():
    rng = np.random.default_rng(77)
    out = []
    tbl = lengths_table(rng)
    text = fasta(tbl)
    # every read length against every contaminant length: the whole contaminant (or the whole read) at the 5' end, half of it at the 3'
    for rl in READ_LENS:
        for name, c in tbl:
            r1, r2 = _rand(rng, rl), _rand(rng, rl)
            k5, k3 = min(len(c), rl), max(min(len(c), rl) // 2, 1)
            for r in (r1, r2):
                r[:k5] = c[len(c) - k5:]
                r[rl - k3:] = c[:k3] if k5 + k3 <= rl else r[rl - k3:]
            out.append((text, 0, 0, r1, r2, "rl%d_%s" % (rl, name)))
    # one contaminant of 200 and a read of 200 that IS its suffix / prefix, with substitutions at chosen places of the overlap
    c200 = _rand(rng, 200)
    t200 = fasta([("whole@1234", c200)])
    for L in (1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 200):
        for where in ("none", "first", "last", "word", "two", "readN", "twoN"):
            r5, r3 = _rand(rng, 220), _rand(rng, 220)
            r5[L] = _other(c200[200 - L - 1]) if L < 200 else r5[L]          # no longer overlap by chance
            r3[220 - L - 1] = _other(c200[L]) if L < 200 else r3[220 - L - 1]
            r5[:L], r3[220 - L:] = c200[200 - L:], c200[:L]
            at = {"none": [], "first": [0], "last": [L - 1], "word": [min(63, L - 1) if L <= 64 else 64], "two": [0, L - 1], "readN": [L // 2],
                  "twoN": [0, L - 1]}[where]
            if L == 1 and where in ("two", "twoN"):
                continue
            for p in at:
                for r, base in ((r5, 0), (r3, 220 - L)):
                    r[base + p] = 4 if where in ("readN", "twoN") else _other(r[base + p])
            out.append((t200, 0, 0, r5, r3, "sub_%s_L%d" % (where, L)))
    # a contaminant N opposite A/C/G/T is free, opposite a read N it costs one
    cn = _rand(rng, 40)
    cn[35], cn[4] = 4, 4
    tn = fasta([("withN@13", cn)])
    for note, n_at_read in (("contamN_free", False), ("contamN_readN", True)):
        r = _rand(rng, 100)
        r[:30], r[70:] = cn[10:], cn[:30]
        r[25] = 4 if n_at_read else 2   # opposite cn[35]
        r[74] = 4 if n_at_read else 1   # opposite cn[4]
        r[3] = _other(r[3])             # and one real substitution: with the read N that makes two at this length
        r[90] = _other(r[90])
        out.append((tn, 0, 0, r, None, note))
    # two contaminants, the SHORTER gives the longer overlap
    ca, cb = _rand(rng, 60), _rand(rng, 30)
    r = _rand(rng, 100)
    r[:10], r[:25] = ca[50:], cb[5:]
    out.append((fasta([("long@1", ca), ("short@1", cb)]), 0, 0, r, None, "shorter_wins"))
    # two substitutions at the longest overlap with a clean shorter one below it: a contaminant of period 5, 30 of it on the read, the
    # substitutions behind base 25; what follows on the read breaks the period
    unit = [0, 1, 2, 3, 3]
    r = unit * 6 + [1, 0, 0, 2, 1] + _rand(rng, 65)
    r[27], r[29] = _other(r[27]), _other(r[29])
    out.append((fasta([("period@1", unit * 8)]), 0, 0, r, None, "two_subs_clean_below"))
    # classes: the reverse complement codes, a PE2-only contaminant that must not touch PE1, a class with 400 entries and one with none
    cr = _rand(rng, 36)
    rcr = [3 - b for b in reversed(cr)]
    r1, r2 = _rand(rng, 90), _rand(rng, 90)
    r1[:20], r1[70:], r2[:20], r2[70:] = rcr[16:], rcr[:20], rcr[16:], rcr[:20]
    out.append((fasta([("rc@5678", cr)]), 0, 0, r1, r2, "revcpl_classes"))
    r1, r2 = _rand(rng, 90), _rand(rng, 90)
    r1[:20], r2[:20], r1[70:], r2[70:] = cr[16:], cr[16:], cr[:20], cr[:20]
    out.append((fasta([("pe2only@24", cr)]), 0, 0, r1, r2, "pe2_only"))
    many = [("m%d@1" % k, _rand(rng, int(rng.integers(4, 60)))) for k in range(400)]
    text400 = fasta(many)
    for k in (0, 199, 399):
        r = _rand(rng, 120)
        c = many[k][1]
        r[:len(c)] = c
        out.append((text400, 0, 0, r, _rand(rng, 120), "class_of_400_entry%d" % k))
    more = many + [("x%d@1" % k, _rand(rng, int(rng.integers(20, 61)))) for k in range(410)]  # 810: three tiles of the kernel's table
    text810 = fasta(more)
    for k in (5, 405, 809):
        r = _rand(rng, 120)
        c = more[k][1]
        r[:len(c)] = c
        out.append((text810, 0, 0, r, None, "class_of_810_entry%d" % k))
    # the end trims: -y3 with an overlap of 3 (contaminant trim 0) and of 5 (2); -Y2 likewise with 2 and 4
    ct = _rand(rng, 20)
    tt = fasta([("t5@1", ct), ("t3@3", ct)])
    ent = R.parse_contaminants(tt)
    for k5, k3 in ((3, 2), (5, 4), (4, 3)):
        while True:  # (random bases beyond the overlaps, drawn until no longer overlap exists by chance)
            r = _rand(rng, 80)
            r[:k5], r[80 - k3:] = ct[20 - k5:], ct[:k3]
            if R.read_trims(ent, r, False, 0, 0) == (k5, k3):
                break
        out.append((tt, 3, 2, r, None, "trims_y3_Y2_overlap%d_%d" % (k5, k3)))
    # the overlap is the whole read: nothing is left (under length, and in PE its mate goes with it)
    c50 = _rand(rng, 50)
    out.append((fasta([("all@1", c50)]), 0, 0, list(c50[10:]), _rand(rng, 60), "whole_read"))
    return out


def expect(note):
    """(contam5, contam3) of PE1 for the cases whose answer is plain by design, else None"""
    if note.startswith("sub_"):
        where, L = note[4:].rsplit("_L", 1)
        if where in ("none", "first", "last", "word", "readN") and int(L) >= 16:
            return int(L), None
    if note == "two_subs_clean_below":
        return 25, None
    if note.startswith("trims_y3_Y2_overlap"):
        k5, k3 = (int(x) for x in note[len("trims_y3_Y2_overlap"):].split("_"))
        return max(k5 - 3, 0), max(k3 - 2, 0)
    if note == "whole_read":
        return 40, None
    return None
