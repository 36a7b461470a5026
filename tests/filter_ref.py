"""kalign's loci base constraints (`-5`) and chromosome filters (`-Z` / `-z`) restated in Python: the two marking rules of
CKAligner::IdentifyConstraintViolations (ngskit4b/KAligner.cpp:2716-2765, AcceptLociConstraints :2647-2714, AcceptBaseConstraint
:2598-2645) and CKAligner::FiltByChroms (:4025-4091), the CSV rules of LoadLociConstraints (:1363-1545) and the accept decision
of CUtility::MatchExcludeRegExpr / MatchIncludeRegExpr (libkit4b/Utility.cpp:226-287).

A record is a dict: nar, num_hits, chrom (1-based entry id), strand, seq (the read as kalign holds it for the test: reverse
complemented for a '-' alignment; codes A0 C1 G2 T3 N4) and segs, a list of (first locus, number of loci, index into seq of the
first locus' base) -- AdjStartLoci, AdjEndLoci - AdjStartLoci + 1 and ReadOfs + TrimLeft of Seg[0] and, for a two-segment read,
Seg[1].  The walk is literal (every locus against every constraint of the sequence); violations_dense does the same through a
per-locus table and is what the 2 M read device test uses.
"""
import re

import numpy as np

NAR_ACCEPTED, NAR_PCRDUP, NAR_CHROMFILT, NAR_LOCICONSTRAINED = 1, 9, 11, 19
BITS = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 16}
MAX_CHROMS, MAX_LOCI = 64, 6400  # cMaxConstrainedChroms, cMaxConstrainedLoci (KAligner.h:92-93)


class ConstraintError(ValueError):
    pass


def _fields(line):
    out, p = [], 0
    while True:
        while p < len(line) and line[p] in " \t":
            p += 1
        if p < len(line) and line[p] in "\"'":
            q = line.find(line[p], p + 1)
            q = len(line) if q < 0 else q
            out.append((line[p + 1:q], True))
            p = line.find(",", q)
            p = len(line) if p < 0 else p
        else:
            q = line.find(",", p)
            q = len(line) if q < 0 else q
            out.append((line[p:q].rstrip(" \t"), False))
            p = q
        if p >= len(line):
            return out
        p += 1


def _is_number(v):
    try:
        float(v)
        return True
    except ValueError:
        return False


def load_constraints(text, names, seq_lens):
    """LoadLociConstraints: [(chrom id, start, end, bits)] sorted; names / seq_lens: the index's sequences in entry order"""
    lower = [n.lower() for n in names]
    out, chroms, n_lines = [], [], 0
    for no, line in enumerate(re.split(r"\r\n|\r|\n", text), 1):
        s = line.lstrip(" \t")
        if not s or s.startswith("#"):
            continue
        f = _fields(s)
        n_lines += 1
        if len(f) < 4:
            raise ConstraintError("Expected at least 4 fields at line %d" % no)
        if n_lines == 1:  # CCSVFile::IsLikelyHeaderLine: no unquoted number, at most two empty fields
            empty = sum(1 for v, q in f if not q and v == "")
            if empty <= 2 and not any(_is_number(v) for v, q in f if not q and v != ""):
                continue
        name = f[0][0]
        if name.lower() not in lower:
            raise ConstraintError("Unable to find matching indexed identifier for '%s' at line %d" % (name, no))
        cid = lower.index(name.lower()) + 1
        atoi = lambda v: int(re.match(r"\s*[-+]?\d*", v).group(0) or 0) if re.match(r"\s*[-+]?\d+", v) else 0  # noqa: E731
        start, end = atoi(f[1][0]), atoi(f[2][0])
        if start < 0 or start > end:
            raise ConstraintError("Start loci must be >= 0 and <= end loci for '%s' at line %d" % (name, no))
        if end >= seq_lens[cid - 1]:
            raise ConstraintError("End loci must be > targeted sequence length for '%s' at line %d" % (name, no))
        bits = 0
        for ch in f[3][0]:
            if ch in " \t":
                continue
            if ch.upper() not in BITS:
                raise ConstraintError("Illegal base specifiers for '%s' at line %d" % (name, no))
            bits |= BITS[ch.upper()]
        if not bits:
            raise ConstraintError("Illegal base specifiers for '%s' at line %d" % (name, no))
        if cid not in chroms:
            if len(chroms) == MAX_CHROMS:
                raise ConstraintError("Number of constrained chroms would be more than max (%d) allowed for '%s' at line %d" % (MAX_CHROMS, name, no))
            chroms.append(cid)
        if len(out) == MAX_LOCI:
            raise ConstraintError("Number of constrained loci would be more than max (%d) allowed for '%s' at line %d" % (MAX_LOCI, name, no))
        out.append((cid, start, end, bits))
    return sorted(out, key=lambda c: c[:3])


def accept_base(table, chrom, loci, base, target_base):
    """AcceptBaseConstraint for a sequence that has constraints: False when a constraint covering loci turns the base down"""
    for cid, start, end, bits in table:
        if cid < chrom:
            continue
        if cid > chrom:
            break
        if start <= loci <= end:
            if bits & 0x10 and target_base(chrom, loci) == base:
                continue
            if base <= 3 and bits & (1 << base):
                continue
            return False
    return True


def accepts(rec, table, target_base):
    """AcceptLociConstraints"""
    if rec["nar"] != NAR_ACCEPTED or not any(c[0] == rec["chrom"] for c in table):
        return True
    for first, n, q in rec["segs"]:
        for j in range(n):
            if not accept_base(table, rec["chrom"], first + j, int(rec["seq"][q + j]), target_base):
                return False
    return True


def _mark(rec, nar):
    rec["nar"], rec["num_hits"], rec["inst"] = nar, 0, 0


def mark_loci_constraints(recs, table, target_base, pe=False):
    """IdentifyConstraintViolations; pe: recs[2i], recs[2i + 1] are mates.  Returns the number of reads marked."""
    if not table:
        return 0
    n = 0
    for i, r in enumerate(recs):
        if r["nar"] == NAR_ACCEPTED and not accepts(r, table, target_base):
            _mark(r, NAR_LOCICONSTRAINED)
            n += 1
        if pe and r["nar"] == NAR_LOCICONSTRAINED and recs[i ^ 1]["nar"] != NAR_LOCICONSTRAINED:
            _mark(recs[i ^ 1], NAR_LOCICONSTRAINED)
            n += 1
    return n


def chrom_accept(names, include=(), exclude=()):
    """per entry id (index 0 unused): False when an exclude expression matches the name up to its first blank, or include
    expressions were given and none matches (std::regex_search; these expressions mean the same to Python's re)"""
    inc, exc = [re.compile(x[:100]) for x in include], [re.compile(x[:100]) for x in exclude]
    out = [False]
    for n in names:
        n = re.split(r"[ \t]", n, 1)[0][:100]
        keep = not any(x.search(n) for x in exc)
        if keep and inc:
            keep = any(x.search(n) for x in inc)
        out.append(keep)
    return out


def mark_chroms(recs, accept):
    """FiltByChroms.  Returns the number of reads marked."""
    n = 0
    for r in recs:
        if r["nar"] == NAR_ACCEPTED and not accept[r["chrom"]]:
            _mark(r, NAR_CHROMFILT)
            n += 1
    return n


# ---- the same bit for many reads: one table per sequence, bit b of fail[chrom][loci] = "base b is turned down at loci" -----------
def fail_tables(table, chroms):
    """chroms: the sequences (uint8 codes, N = 4) in entry order"""
    out = {}
    for cid, start, end, bits in table:
        t = out.setdefault(cid, np.zeros(len(chroms[cid - 1]), np.uint8))
        tb = np.asarray(chroms[cid - 1][start:end + 1], np.uint8)
        f = np.zeros(end + 1 - start, np.uint8)
        for b in range(5):
            ok = np.full(len(f), bool(b <= 3 and bits & (1 << b)))
            if bits & 0x10:
                ok |= tb == b
            f |= np.where(ok, 0, 1 << b).astype(np.uint8)
        t[start:end + 1] |= f
    return out


def violations_dense(table, chroms, chrom, seg_first, seg_n, seg_q, minus, reads, offs, lens, accepted, chunk=200_000):
    """bool per read: accepted and some locus of one of its segments fails.  chrom / minus / offs / lens / accepted: per read;
    seg_first / seg_n / seg_q: [2, n] (n = 0: no such segment); reads: the bases as sequenced (low 3 bits), concatenated."""
    n = len(chrom)
    fail = fail_tables(table, chroms)
    lens_c = np.array([len(c) for c in chroms], np.int64)
    base = np.concatenate([[0], np.cumsum(lens_c)])
    dense = np.zeros(int(base[-1]), np.uint8)
    for cid, t in fail.items():
        dense[base[cid - 1]:base[cid]] = t
    con = np.zeros(len(chroms) + 2, bool)
    con[list(fail)] = True
    out = np.zeros(n, bool)
    for sg in range(2):
        for a in range(0, n, chunk):
            idx = a + np.flatnonzero(accepted[a:a + chunk] & con[chrom[a:a + chunk]] & (seg_n[sg][a:a + chunk] > 0))
            if not len(idx):
                continue
            cnt = seg_n[sg][idx].astype(np.int64)
            rid = np.repeat(np.arange(len(idx)), cnt)
            j = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            loci = seg_first[sg][idx][rid].astype(np.int64) + j
            q = seg_q[sg][idx][rid].astype(np.int64) + j
            ln = lens[idx][rid].astype(np.int64)
            inside = q < ln
            src = offs[idx][rid].astype(np.int64) + np.where(minus[idx][rid], ln - 1 - q, q)
            b = np.where(inside, reads[np.where(inside, src, 0)] & 7, 4).astype(np.int64)
            b = np.where(minus[idx][rid] & (b <= 3), 3 - b, b)
            b = np.minimum(b, 4)
            bad = (dense[base[chrom[idx] - 1][rid] + loci] >> b) & 1
            out[idx] |= np.add.reduceat(bad.astype(np.int64), np.cumsum(cnt) - cnt) > 0  # (every cnt is positive)
    return out
