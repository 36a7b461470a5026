"""kalign's contaminant flank trimming (`-H <file>`) restated by brute force, for the tests of k4_contam.hip and `k4align -H`.

Written from the behaviour of the reference (CContaminants::LoadContaminantsFile / MatchContaminants in libkit4b/Contaminants.cpp and
their use in CKAligner::LoadRawReads, ngskit4b/KAligner.cpp:11992-12290), not from the project's C++: sequences are plain Python
lists, an overlap is compared base by base.

Bases are etSeqBase codes: A=0 C=1 G=2 T=3 N=4, '-' = 6.  Classes: 0 5' of SE/PE1, 1 5' of PE2, 2 3' of SE/PE1, 3 3' of PE2."""
MIN_CONTAM, MAX_CONTAM, MAX_ENTRIES = 4, 200, 1600
MIN_READ, MAX_READ = 20, 2000


class Refused(Exception):
    """the reference turns the file down"""


class Vector(Exception):
    """the file holds a `&` (vector, containment) record: out of scope"""


def codes(text):
    """letters -> base codes, as CFasta does: acgtu either case, '-' 6, any other letter N"""
    out = []
    for ch in text:
        k = "ACGT".find(ch.upper()) if ch.upper() != "U" else 3
        out.append(k if k >= 0 else 6 if ch == "-" else 4)
    return out


def letters(bases):
    return "".join("ACGTN"[b] if b <= 4 else "-" for b in bases)


def _classes_of(descr, seq_id):
    """(name, eight flags, is vector) of a descriptor line without its '>'"""
    words = descr[:105].split()
    dflt = [True, True, False, False, True, True, False, False]
    if not words:
        return "ContamSeq.%d" % seq_id, dflt, False
    name = words[0]
    p = len(name) - 1
    while p >= 1 and "1" <= name[p] <= "8":  # the first character is never passed over
        p -= 1
    vector = name[p] == "&"
    if name[p] in "@&" and p + 1 < len(name):
        flags = [str(k + 1) in name[p + 1:] for k in range(8)]
        return name[:p][:80], flags, vector
    return name[:80], dflt, vector


def parse_contaminants(data):
    """the file's bytes -> [(cls, bases, name, revcpl)] in the order the reference adds them"""
    text = data.decode("latin-1")
    recs = []  # (descriptor or None, sequence letters)
    cur_descr, seq, pos, owes = None, [], 0, False
    while pos <= len(text):
        ch = text[pos] if pos < len(text) else ">"
        if ch == ">":
            if seq or owes:
                recs.append((cur_descr, "".join(seq) if seq else "N"))  # a descriptor with nothing behind it is given one N
            seq, owes = [], False
            if pos == len(text):
                break
            end = pos + 1
            while end < len(text) and text[end] not in "\r\n":
                end += 1
            cur_descr, owes = text[pos + 1:end].lstrip(" \t"), True
            pos = end
            continue
        if ch.isalpha() and ch.isascii() or ch == "-":
            seq.append(ch)
        pos += 1
    entries = []
    seq_id, vector = 0, False

    def add(cls, bases, name, rc):
        if len(entries) >= MAX_ENTRIES:
            raise Refused("Too many flank contaminants")
        for c, b, n, _ in entries:
            if c == cls and (n.lower() == name.lower() or b == bases):
                raise Refused("duplicated")
        entries.append((cls, bases, name, rc))

    for descr, s in recs:
        if descr is not None:
            seq_id += 1
            name, flags, vector = _classes_of(descr, seq_id)
        elif not seq_id:
            seq_id, name, flags = 1, "ContamSeq.1", [True, True, False, False, True, True, False, False]
        if vector:
            raise Vector(name)
        if not MIN_CONTAM <= len(s) <= MAX_CONTAM:
            raise Refused("outside of accepted length range")
        bases = codes(s)
        if any(b > 4 for b in bases):
            raise Refused("Illegal base")
        for c in range(4):
            if flags[c]:
                add(c, bases, name, False)
        if any(flags[4:]):
            rc = [3 - b if b < 4 else b for b in reversed(bases)]
            for c in range(4):
                if flags[4 + c]:
                    add(c, rc, name + "xRC", True)
    if not entries:
        raise Refused("No Contaminants loaded")
    return entries


def overlap_ok(contam, read, L, five):
    """at most one substitution between the contaminant's last (5') / first (3') L bases and the read's first / last L"""
    subs = 0
    for k in range(L):
        c = contam[len(contam) - L + k] if five else contam[k]
        r = (read[k] if five else read[len(read) - L + k]) & 7
        if r == 4 or (c != 4 and r != c):
            subs += 1
            if subs > 1:
                return False
    return True


def match(entries, cls, min_overlap, read):
    """MatchContaminants: the largest accepted overlap, 0 for none"""
    if not MIN_READ <= len(read) <= MAX_READ:
        return 0
    mine = [b for c, b, _, _ in entries if c == cls]
    if not mine:
        return 0
    five = cls < 2
    for L in range(min(len(read), max(len(b) for b in mine)), max(min_overlap, 1) - 1, -1):
        if any(len(b) >= L and overlap_ok(b, read, L, five) for b in mine):
            return L
    return 0


def read_trims(entries, read, pe2, trim5, trim3):
    """(contam5, contam3) of one read: what LoadRawReads takes off beyond -y / -Y"""
    l5 = match(entries, 1 if pe2 else 0, trim5 + 1, read)
    l3 = match(entries, 3 if pe2 else 2, trim3 + 1, read)
    return max(l5 - trim5, 0), max(l3 - trim3, 0)


def load_reads(entries, reads1, reads2=None, trim5=0, trim3=0, min_len=50, max_len=500, sample_nth=1):
    """LoadRawReads over the reads (PE: reads2 the mates) -> dict:
    kept   [(unit index, [(start, end) of the stored part of each end])], in load order
    trims  [per unit [(contam5, contam3) per end]] (None for a unit -# passes over)
    under, over, totals [5' PE1, 3' PE1, 5' PE2, 3' PE2 among the kept]"""
    kept, trims, under, over, totals = [], [], 0, 0, [0, 0, 0, 0]
    for i, r1 in enumerate(reads1):
        if sample_nth > 1 and i % sample_nth:  # every n-th unit of the file, the first included; the others are never looked at
            trims.append(None)
            continue
        ends = [r1] + ([reads2[i]] if reads2 is not None else [])
        t = [read_trims(entries, r, e == 1, trim5, trim3) if entries else (0, 0) for e, r in enumerate(ends)]
        trims.append(t)
        verdict = None
        for r, (c5, c3) in zip(ends, t):  # PE1 under, PE1 over, PE2 under, PE2 over
            if trim5 + trim3 + c5 + c3 + min_len > len(r):
                verdict = "under"
            elif trim5 + trim3 + c5 + c3 + max_len < len(r):
                verdict = "over"
            if verdict:
                break
        if verdict == "under":
            under += 1
            continue
        if verdict == "over":
            over += 1
            continue
        kept.append((i, [(trim5 + c5, len(r) - trim3 - c3) for r, (c5, c3) in zip(ends, t)]))
        for e, (c5, c3) in enumerate(t):
            totals[2 * e] += c5 > 0
            totals[2 * e + 1] += c3 > 0
    return dict(kept=kept, trims=trims, under=under, over=over, totals=totals)


def match_many(entries, cls, min_overlap, reads):
    """match() for many reads of ONE length at once (reads: 2-D array of base codes): the same comparisons, made array by array"""
    import numpy as np

    reads = np.asarray(reads, dtype=np.uint8) & 7
    n, rl = reads.shape
    best = np.zeros(n, dtype=np.int64)
    mine = [np.array(b, dtype=np.uint8) for c, b, _, _ in entries if c == cls]
    if not mine or not MIN_READ <= rl <= MAX_READ:
        return best
    five = cls < 2
    for L in range(min(rl, max(len(b) for b in mine)), max(min_overlap, 1) - 1, -1):
        todo = best == 0
        if not todo.any():
            break
        part = reads[todo, :L] if five else reads[todo, rl - L:]
        ok = np.zeros(part.shape[0], dtype=bool)
        for b in mine:
            if len(b) >= L:
                c = b[len(b) - L:] if five else b[:L]
                ok |= ((part == 4) | ((c != 4) & (part != c))).sum(axis=1) <= 1
        idx = np.flatnonzero(todo)[ok]
        best[idx] = L
    return best
