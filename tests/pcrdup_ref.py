"""A literal Python restatement of kalign's PCR artefact reduction (`-k <WinLen>`): CKAligner::ReducePCRduplicates
(ngskit4b/KAligner.cpp:2303-2400), NumUpUniques / NumDnUniques (:10714-10830) over the reads in SortHitMatch order (:10969-11015)
with ties in load order -- what the reference does when it runs one thread.  The index arithmetic follows the C step for step
(ReadHitIdx is 1-based, SortReadHits).  It checks the device stage (kit4b_amd/csrc/k4_pcrdup.hip) and the golden runs.

A record is a dict with nar, num_hits, chrom, start (AdjStartLoci), len (AdjHitLen), strand ('+' / '-'), low_mm; the list is in
load order.  reduce_pcr_duplicates() changes the records in place and returns the number of reads it marked.
"""
NAR_ACCEPTED, NAR_PCRDUP = 1, 9


def sort_hit_match(recs):
    """the reads' order after SortReadHits(eRSMHitMatch): NAR, NumHits (1, then 0, 2, 3, ...), chrom, start, length, strand, LowMMCnt;
    a pair SortHitMatch calls equal keeps its load order"""
    def key(i):
        r = recs[i]
        if r["num_hits"] != 1:
            return (r["nar"], 1, r["num_hits"], 0, 0, 0, 0, 0)
        return (r["nar"], 0, 0, r["chrom"], r["start"], r["len"], ord(r["strand"]), r["low_mm"])
    return sorted(range(len(recs)), key=key)  # (Python's sort is stable: load order within equal keys)


def num_dn_uniques(idx, recs, cur, win_len):
    n_loaded = len(idx)
    nxt = recs[cur]["read_hit_idx"]
    if nxt == n_loaded:
        return 0
    cur_chrom, cur_start, cur_strand = recs[cur]["chrom"], recs[cur]["start"], recs[cur]["strand"]
    prv = cur_start
    n = 0
    while True:
        r = recs[idx[nxt]]
        nxt = r["read_hit_idx"]
        if cur_chrom != r["chrom"]:
            return n
        if r["nar"] == NAR_ACCEPTED:
            s = r["start"]
            if cur_start + win_len < s:
                return n
            if cur_strand == r["strand"] and s != prv:
                n += 1
                prv = s
        if nxt == n_loaded:
            return n


def num_up_uniques(idx, recs, cur, win_len):
    nxt = recs[cur]["read_hit_idx"]
    if nxt == 1:
        return 0
    cur_chrom, cur_start, cur_strand = recs[cur]["chrom"], recs[cur]["start"], recs[cur]["strand"]
    prv = cur_start
    n = 0
    while True:
        r = recs[idx[nxt - 1]]
        if cur_chrom != r["chrom"]:
            return n
        if r["nar"] == NAR_ACCEPTED:
            s = r["start"]
            if cur_start > win_len and cur_start - win_len > s:
                return n
            if cur_strand == r["strand"] and s != prv:
                n += 1
                prv = s
        nxt -= 1
        if nxt <= 0:
            return n


def limit_of(up, dn, win_len):
    lim = max(up, dn)
    prop = int((float(lim) / win_len) * 100.0)
    return 1 if prop < 5 else 2 if prop <= 10 else 3 if prop <= 20 else 4 if prop <= 40 else 5 if prop <= 60 else 10 if prop <= 80 else 50


def reduce_pcr_duplicates(recs, win_len):
    idx = sort_hit_match(recs)
    for k, i in enumerate(idx):
        recs[i]["read_hit_idx"] = k + 1
    n_dups = 0
    p = 0  # position in idx of the read IterSortedReads returns next
    while p < len(idx):
        cur = idx[p]
        if recs[cur]["nar"] != NAR_ACCEPTED:
            p += 1
            continue
        if win_len > 0:
            limit = limit_of(num_up_uniques(idx, recs, cur, win_len), num_dn_uniques(idx, recs, cur, win_len), win_len)
        else:
            limit = 0
        mark = p
        c = recs[cur]
        q = p + 1
        while q < len(idx):
            r = recs[idx[q]]
            if r["nar"] != NAR_ACCEPTED:
                q += 1
                continue
            if c["chrom"] == r["chrom"] and c["start"] == r["start"] and c["strand"] == r["strand"]:
                if c["len"] != r["len"]:
                    q += 1
                    continue
                if limit > 0:
                    limit -= 1
                    q += 1
                    continue
                r["num_hits"] = 0
                r["inst"] = 0
                r["nar"] = NAR_PCRDUP
                mark = q
                n_dups += 1
                q += 1
            else:
                break
        p = mark + 1
    return n_dups
