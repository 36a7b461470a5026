"""A restatement of kalign's priority regions (`-B <bed>`, `-V`) for the tests: the BED reader's interval semantics
(CBEDfile::ProcessBedFile / AddFeature / InAnyFeature, libkit4b/BEDfile.cpp:1172-1327, 1794-2055, 3247-3306, 3991), the priority pass
of CKAligner::ProcCoredApprox (ngskit4b/KAligner.cpp:9682-9770) over two AlignRead passes of the oracle, and FiltByPriorityRegions
(:4093-4155).  Literal and sequential; no device."""
import numpy as np

PRIORITY_EXACTS = 10  # cPriorityExacts, KAligner.h:58
NAR_ACCEPTED, NAR_MULTIALIGN, NAR_REGIONFILT = 1, 5, 12
HR_HITS = 1


def read_bed(text):
    """[(name, start, inclusive end)] of a BED text: white space between the fields, '#' and blank lines sloughed, lines that do not
    parse sloughed while no feature was read (track lines, titles); End - 1 is kept (AddFeature :2055)"""
    feats, n = [], 0
    for line in text.splitlines():
        t = line.strip()
        if not t or t.startswith("#"):
            continue
        f = t.split()
        try:
            name, s, e = f[0], int(f[1]), int(f[2])
        except (IndexError, ValueError):
            if n == 0:
                continue
            raise ValueError("not a BED line: %r" % line)
        if s < 0 or e < s:
            raise ValueError("feature %d..%d" % (s, e))
        n += 1
        if e > 0:  # (0..0: End = -1 meets no span)
            feats.append((name[:80], s, e - 1))  # start == end: a feature of no bases, kept with End = Start - 1
    if n == 0:
        raise ValueError("no feature")
    return feats


def locate_chrom(bed_names, name):
    """LocateChromIDbyName (:3070-3095): without regard to case, chloroplast = ChrC and mitochondria = ChrM"""
    low = {}
    for k, b in enumerate(bed_names):
        low.setdefault(b.lower(), k)
    q = name.lower()
    if q in low:
        return low[q]
    for a, b in (("chloroplast", "chrc"), ("mitochondria", "chrm"), ("chrc", "chloroplast"), ("chrm", "mitochondria")):
        if q == a and b in low:
            return low[b]
    return -1


class Regions:
    """the features per sequence of the index (entry ids are 1-based)"""

    def __init__(self, bed_text, index_names):
        feats = read_bed(bed_text)
        names = []
        for f in feats:
            if f[0].lower() not in [n.lower() for n in names]:
                names.append(f[0])
        self.by_entry = {}
        for c, nm in enumerate(index_names, 1):
            k = locate_chrom(names, nm)
            if k >= 0:
                self.by_entry[c] = [(s, e) for (b, s, e) in feats if b.lower() == names[k].lower()]

    def in_any_feature(self, chrom_id, start, end):
        """InAnyFeature: a feature of the sequence with Start <= end and End >= start (inclusive loci, any strand)"""
        return any(s <= end and e >= start for s, e in self.by_entry.get(int(chrom_id), ()))

    def hit_in_feature(self, h):
        return self.in_any_feature(h["chrom_id"], int(h["match_loci"]), int(h["match_loci"]) + int(h["match_len"]) - 1)

    def mask(self, hits):
        """hit_in_feature over an array of hit records of any shape, at once"""
        c = hits["chrom_id"].astype(np.int64)
        s = hits["match_loci"].astype(np.int64)
        e = s + hits["match_len"].astype(np.int64) - 1
        m = np.zeros(hits.shape, bool)
        for cid, iv in self.by_entry.items():
            on = c == cid
            for fs, fe in iv:
                m |= on & (fs <= e) & (fe >= s)
        return m

    def intervals(self):
        """(entry ids, starts, ends) as k4_set_priority_regions takes them"""
        t = [(c, s, e) for c, iv in sorted(self.by_entry.items()) for s, e in iv]  # (a feature of no bases goes as end = start - 1)
        return [np.array(x, np.uint32) for x in (zip(*t) if t else ((), (), ()))]


def select(regions, wide_out, wide_hits, norm_out, norm_hits, max_ml, pe_mode=0):
    """The priority pass over the records of two AlignRead passes: wide = with max_ml + 10 hits (no microInDel / splice), norm = the
    normal call.  Returns (out, hits, needs_normal)."""
    n = len(wide_out)
    out, hits = norm_out.copy(), norm_hits.copy()
    need = np.ones(n, bool)
    pri = regions.mask(wide_hits)
    for i in range(n):
        w = wide_out[i]
        if w["hit_rslt"] != HR_HITS:
            continue
        # :9732-9755 literally: the slot a priority hit is copied to moves with the copies only, and nothing is copied before a hit
        # outside the regions has been passed -- [P1, N, P2] becomes [P2, N, P2] with two instances
        multi = wide_hits[i].copy()
        k = n_out = dst = 0
        for q in range(min(int(w["inst"]), max_ml + PRIORITY_EXACTS)):
            if not pri[i, q]:
                n_out += 1
                continue
            if n_out > 0:
                multi[dst] = wide_hits[i, q]
                dst += 1
            k += 1
        if not (0 < k <= max_ml):
            continue
        need[i] = False
        hits[i] = np.zeros(max_ml, hits.dtype)
        hits[i, :k] = multi[:k]
        if pe_mode >= 2:
            nar, nh = NAR_ACCEPTED, k
        elif pe_mode == 0 or k == 1:
            nar, nh = NAR_ACCEPTED, 1
        else:
            nar, nh = NAR_MULTIALIGN, k
        out[i] = (HR_HITS, k, w["low_mm"], w["nxt_mm"], nar, nh)
    return out, hits, need


def filter_regions(regions, nar, num_hits, hits0):
    """FiltByPriorityRegions over flat arrays (hits0 = the reported hit of every read), in place; returns the number marked"""
    cnt = 0
    for i in range(len(nar)):
        if nar[i] == NAR_ACCEPTED and not regions.hit_in_feature(hits0[i]):
            nar[i], num_hits[i] = NAR_REGIONFILT, 0
            hits0[i]["chrom_id"] = 0
            cnt += 1
    return cnt
