"""Restatement of kalign's per-target PE insert length table (`-3`): CKAligner::ReportPEInsertLenDist over the order of
SortPEHitMatch, and MedianInsertLen (ngskit4b/KAligner.cpp:5255-5454, 10928-10963), over records in k4_pe_read layout
(kit4b_amd.PE_READ_DTYPE, mates at 2q and 2q + 1).

walk_literal is the reference's loop statement by statement, for small inputs.  collect does the same walk with numpy where the
reference has per-read arithmetic (the sort, TLen, the columns), so that a million pairs take seconds; the test compares the two.
median_insert_len is MedianInsertLen's loop as written; its inner loop computes NumUnder / NumOver, which depend on the candidate's
value alone, so they are counted once per distinct value and remembered (the reference recounts them for every candidate).
"""
import numpy as np

MAX_PAIRS = 1000000
NAR_ACCEPTED = 1
U32 = 0xFFFFFFFF


def bin_of(tlen):
    if tlen < 100:
        return 0
    if tlen > 600:
        return 51
    return 1 + (tlen - 99) // 10


def median_insert_len(lens):
    n = len(lens)
    if n == 0:
        return 0
    if n == 1:
        return int(lens[0])
    if n == 2:
        return ((int(lens[0]) + int(lens[1])) & U32) // 2
    arr = np.asarray(lens, np.uint32)
    vals = arr.tolist()
    lo = hi = 0
    for v in vals:
        if v < lo or lo == 0:
            lo = v
        if v > hi or hi == 0:
            hi = v
    if hi == lo:
        return hi
    counted = {}
    for idx in range(1, n):
        cur = vals[idx]
        if cur < lo or cur > hi:
            continue
        if cur not in counted:  # over every other element that differs from cur: how many lie under it, how many over
            counted[cur] = (int(np.count_nonzero(arr < cur)), int(np.count_nonzero(arr > cur)))
        under, over = counted[cur]
        if under == over:
            return cur
        if under < over:
            lo = cur
        else:
            hi = cur
    return ((lo + hi) & U32) // 2


def _adj(hit):
    """(AdjAlignStartLoci, AdjAlignHitLen) of hits in HIT_DTYPE: the span left inside the trimmed flanks, 32-bit unsigned"""
    ext = hit["reserved"].astype(np.int64)
    tl, tr = ext & 0xFFF, (ext >> 12) & 0xFFF
    plus = hit["strand"] == ord("+")
    start = (hit["match_loci"].astype(np.int64) + np.where(plus, tl, tr)) & U32
    length = (hit["match_len"].astype(np.int64) - tl - tr) & U32
    return start, length


def _tlen(s1, l1, s2, l2):
    s1, s2 = (s1 + 1) & U32, (s2 + 1) & U32
    return np.where(s1 <= s2, ((s2 - s1) & U32) + l2, ((s1 - s2) & U32) + l1) & U32


def _sorted_reads(pe):
    """indices of the accepted PE-aligned reads in SortPEHitMatch order: target, pair ordinal, PE1 before PE2"""
    sel = np.flatnonzero((pe["nar"] == NAR_ACCEPTED) & (pe["pe_aligned"] != 0))
    return sel[np.argsort(pe["hit"]["chrom_id"][sel], kind="stable")]


def walk_literal(pe):
    """rows [(chrom, NumPEs, median, sum, [52 columns])] by the reference's loop, one pair of sorted elements at a time"""
    order = _sorted_reads(pe)
    start, length = _adj(pe["hit"])
    rows, cur, num, tot, dist, kept = [], 0, 0, 0, [0] * 52, []

    def close():
        if cur and num:
            rows.append((cur, num, median_insert_len(kept[:MAX_PAIRS]), tot, list(dist)))

    k = 0
    while k + 1 < len(order):
        e1, e2 = order[k], order[k + 1]
        k += 2
        chrom = int(pe["hit"]["chrom_id"][e1])
        if chrom != cur:
            close()
            cur, num, tot, dist, kept = chrom, 0, 0, [0] * 52, []
        if num >= MAX_PAIRS:
            continue
        t = int(_tlen(start[e1], length[e1], start[e2], length[e2]))
        tot += t
        dist[bin_of(t)] += 1
        kept.append(t)
        num += 1
    close()
    return rows


def collect(pe):
    """the same table as arrays: entry_id, tot_pes, median (uint32), sum (uint64), dist [n_rows, 52]"""
    order = _sorted_reads(pe)
    n = len(order) // 2  # a last odd element has no partner
    e1, e2 = order[0:2 * n:2], order[1:2 * n:2]
    start, length = _adj(pe["hit"])
    tlen = _tlen(start[e1], length[e1], start[e2], length[e2])
    chrom = pe["hit"]["chrom_id"][e1]
    heads = np.flatnonzero(np.concatenate([[True], chrom[1:] != chrom[:-1]])) if n else np.zeros(0, np.int64)
    ends = np.concatenate([heads[1:], [n]]).astype(np.int64)
    out = dict(entry_id=chrom[heads].astype(np.uint32), tot_pes=np.zeros(len(heads), np.uint32), median=np.zeros(len(heads), np.uint32),
               sum=np.zeros(len(heads), np.uint64), dist=np.zeros((len(heads), 52), np.uint32))
    for r, (a, b) in enumerate(zip(heads, ends)):
        t = tlen[a:min(b, a + MAX_PAIRS)]  # later pairs of the target are passed over altogether
        col = np.where(t < 100, 0, np.where(t > 600, 51, 1 + (np.maximum(t, 99) - 99) // 10))
        out["tot_pes"][r] = len(t)
        out["sum"][r] = int(t.sum())
        out["dist"][r] = np.bincount(col, minlength=52)
        out["median"][r] = median_insert_len(t)
    return out


def text(rows, names, seq_lens, n_accepted):
    """the file: rows as collect returns them"""
    if not n_accepted:
        return ""
    o = '"TargSeq","TargLen","TotPEs","MedianInsertLen","MeanInsertLen","Insert <100bp"'
    o += "".join(',"Insert %dbp"' % (100 + 10 * k) for k in range(50)) + ',"Insert >600bp"\n'
    for r in range(len(rows["entry_id"])):
        e = int(rows["entry_id"][r]) - 1
        o += '"%s",%d,%d,%d,%d' % (names[e], seq_lens[e], rows["tot_pes"][r], rows["median"][r], int(rows["sum"][r]) // int(rows["tot_pes"][r]))
        o += "".join(",%d" % c for c in rows["dist"][r]) + "\n"
    return o
