"""A literal restatement of what `kalign -8 <file> -9 <ofs>` counts and prints (ngskit4b/KAligner.cpp): the walk of
ProcessSiteProbabilites :8750-8821, its scale step :8823-8872 and WriteSitePrefs :8910-8945.

A record is a dict: chrom (1-based entry id), loci (the RAW Seg[0].MatchLoci), mlen (the raw MatchLen), strand ('+' / '-'), segs
(FlgInDel or FlgSplice); the walk takes the ACCEPTED reads in SortHitMatch order (sort_records, or the order of a SAM body).
`genome` is a list of numpy uint8 arrays of etSeqBase codes, entry order.

walk() is the loop as the reference has it, uint32 arithmetic through `& 0xffffffff`.  A read whose signed locus lies in -8..-1
makes the reference read an uninitialised array: walk() raises Undefined, or passes over the read when told to.
walk_arrays() is the same count in numpy for millions of records; tests/test_siteprefs_cpu.py holds the two together.
"""
import numpy as np

N_OCT = 65536
M32 = 0xFFFFFFFF


class Undefined(Exception):
    """the reference has no behaviour here: GetSeq returned no bases and the octamer is read from an uninitialised array"""


def sort_records(recs):
    """accepted records in load order -> SortHitMatch order (KAligner.cpp:10969): chrom, AdjStartLoci, AdjHitLen, strand, mismatches;
    Python's sort is stable, ties stay in load order"""
    def key(r):
        tl, tr = r.get("tl", 0), r.get("tr", 0)
        return (r["chrom"], r["loci"] + (tl if r["strand"] == "+" else tr), r["mlen"] - tl - tr, ord(r["strand"]), r.get("mm", 0))
    return sorted(recs, key=key)


def hit_loci(loci, mlen, strand, ofs, chrom_len):
    """(HitLoci, defined?) :8766-8782"""
    hl = loci & M32
    if strand == "+":
        hl = (hl + ofs) & M32
    else:
        hl = (hl + mlen - 1) & M32
        hl = (hl - ofs) & M32
        hl = (hl - 7) & M32
    # `if(HitLoci < 0)` never holds for a uint32_t
    if ((hl + 8) & M32) >= (chrom_len & M32):
        hl = (chrom_len - 9) & M32
    got = 0 if hl >= chrom_len else min(8, chrom_len - hl)  # CSfxArray::GetSeq, SfxArray.cpp:2396-2424
    return hl, got == 8


def walk(recs, genome, ofs, skip_undefined=False):
    """NumOccs, NumSites: int64 [2, 65536] (strand, octamer)"""
    occ = np.zeros((2, N_OCT), np.int64)
    sites = np.zeros((2, N_OCT), np.int64)
    prev_entry, prev_loci, chrom_len = 0, M32, M32
    for r in recs:
        if r.get("segs"):
            continue
        if r["chrom"] != prev_entry:
            prev_entry = r["chrom"]
            prev_loci = M32
            chrom_len = len(genome[r["chrom"] - 1])
        hl, defined = hit_loci(r["loci"], r["mlen"], r["strand"], ofs, chrom_len)
        if not defined:
            if skip_undefined:
                continue
            raise Undefined("chrom %d loci %d strand %s" % (r["chrom"], r["loci"], r["strand"]))
        seq = [int(b) & 7 for b in genome[r["chrom"] - 1][hl:hl + 8]]
        strand = 0
        if r["strand"] == "-":
            strand = 1
            seq = [3 - b if b <= 3 else b for b in reversed(seq)]  # CSeqTrans::ReverseComplement
        idx, n = 0, 0
        for b in seq:
            if b > 3:
                break
            idx = (idx << 2) | b
            n += 1
        if n != 8:
            continue
        occ[strand, idx] += 1
        if hl != prev_loci:
            sites[strand, idx] += 1
            prev_loci = hl
    return occ, sites


def walk_arrays(chrom, loci, mlen, minus, segs, genome, ofs):
    """walk(..., skip_undefined=True) over numpy columns in walk order"""
    chrom, loci, mlen = np.asarray(chrom, np.int64), np.asarray(loci, np.int64), np.asarray(mlen, np.int64)
    minus, segs = np.asarray(minus, bool), np.asarray(segs, bool)
    clens = np.array([len(g) for g in genome], np.int64)
    base = np.concatenate([[0], np.cumsum(clens)])
    concat = np.concatenate([np.asarray(g, np.uint8) & 7 for g in genome] + [np.full(8, 7, np.uint8)]).astype(np.int64)
    n_pos = int(base[-1])
    code, clean = np.zeros(n_pos, np.int64), np.ones(n_pos, bool)
    for q in range(8):
        b = concat[q:q + n_pos]
        code = (code << 2) | (b & 3)
        clean &= b <= 3
    hl = np.where(minus, loci + mlen - 1 - ofs - 7, loci + ofs) & M32
    cl = clens[chrom - 1]
    hl = np.where(((hl + 8) & M32) >= cl, (cl - 9) & M32, hl)
    ok = ~segs & (hl < cl) & (cl - hl >= 8)
    pos = np.where(ok, base[chrom - 1] + hl, 0)
    ok &= clean[pos]
    oct_ = code[pos]
    rc = ~oct_ & 0xFFFF
    rc = ((rc & 0x00FF) << 8) | (rc >> 8)
    rc = ((rc & 0x0F0F) << 4) | ((rc >> 4) & 0x0F0F)
    rc = ((rc & 0x3333) << 2) | ((rc >> 2) & 0x3333)
    key = np.where(minus, N_OCT + rc, oct_)[ok]
    site = (chrom[ok] << 32) | hl[ok]
    head = np.ones(len(site), bool)
    head[1:] = site[1:] != site[:-1]
    occ = np.bincount(key, minlength=2 * N_OCT).reshape(2, N_OCT)
    sites = np.bincount(key[head], minlength=2 * N_OCT).reshape(2, N_OCT)
    return occ.astype(np.int64), sites.astype(np.int64)


def scale(occ, sites, reverse_ties=False):
    """RelScale of one strand (:8823-8872).  The reference sorts ascending by NumOccs / NumSites with an unstable quicksort; the rule
    here is a stable sort, ties by octamer ascending (reverse_ties: descending, to show where the rule matters)."""
    rel = [float(occ[k]) / float(sites[k]) if sites[k] >= 1 else 0.0 for k in range(N_OCT)]
    order = sorted(range(N_OCT), key=(lambda k: (rel[k], -k)) if reverse_ties else (lambda k: rel[k]))
    top = 0.0
    for q in range(0xFFC0, N_OCT):
        top += rel[order[q]]
        rel[order[q]] = 1.0
    top /= 64
    for q in range(0xFFC0):
        k = order[q]
        if rel[k] > 0.0:
            rel[k] = max(0.0001, rel[k] / top)
    return rel


def octamer_text(k):
    return "".join("acgt"[(k >> (14 - 2 * q)) & 3] for q in range(8))


def text(occ, sites, n_accepted, reverse_ties=False):
    """the file (:8910-8945); empty when no read was accepted (:743, :780)"""
    if not n_accepted:
        return ""
    out = ['"Id","Strand","Octamer","TotalHits","UniqueLoci","RelScale"\n']
    for strand in (0, 1):
        rel = scale(occ[strand], sites[strand], reverse_ties)
        for k in range(0xFFFF):  # one short of 65536: tttttttt is never written
            out.append('%d,"%s","%s",%d,%d,%1.3f\n' % (k + 1, "+-"[strand], octamer_text(k), occ[strand][k], sites[strand][k], rel[k]))
    return "".join(out)


def boundary_untied(occ, sites):
    """is the outcome of one strand independent of the order of tied entries?  The 64th and 65th largest ratios differ, or all of
    the top 64 equal the 65th and it is non-zero."""
    rel = sorted((float(occ[k]) / float(sites[k]) if sites[k] >= 1 else 0.0 for k in range(N_OCT)), reverse=True)
    return rel[63] != rel[64] or (rel[0] == rel[64] and rel[64] != 0.0)


def records_of_sam(sam_text, names):
    """the accepted alignments of a SAM body, in file order = walk order: raw locus = POS - 1 - leading soft clip, raw length =
    the read's length; a record with N / I / D in its CIGAR is a two-segment read"""
    import re

    ident = {n: i + 1 for i, n in enumerate(names)}
    recs = []
    for line in sam_text.split("\n"):
        if not line or line.startswith("@"):
            continue
        f = line.split("\t")
        if int(f[1]) & 4:
            continue
        ops = re.findall(r"(\d+)([A-Z])", f[5])
        lead = int(ops[0][0]) if ops[0][1] == "S" else 0
        recs.append(dict(chrom=ident[f[2]], loci=int(f[3]) - 1 - lead, mlen=len(f[9]), strand="-" if int(f[1]) & 16 else "+",
                         segs=any(o in "NID" for _, o in ops), clipped=any(o == "S" for _, o in ops)))
    return recs
