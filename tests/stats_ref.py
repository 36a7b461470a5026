"""A literal restatement of what `kalign -O` counts and prints (ngskit4b/KAligner.cpp): WriteSubDist :6469-6525,
WriteBasicCountStats :4159-4300, ReportTargHitCnts :5458-5712, the insert size file of ProcessPairedEnds :3092-3146 and the
tallies m_MultiHitDist :9943 / m_pLenDist :3251, :3408, :3511.

A record is a dict: nar, chrom (1-based entry id), loci (Seg[0].MatchLoci), mlen (MatchLen), strand ('+' / '-'), tl / tr
(TrimLeft / TrimRight), segs (FlagSegs: a two-segment hit), read (numpy uint8: etSeqBase in bits 0..2, the 4-bit quality score in
bits 4..7, in the orientation the read was loaded in).  `genome` is a list of numpy uint8 arrays of etSeqBase codes, entry order.
"""
import numpy as np

NAR_ACCEPTED = 1
MAX_MULTI, PAIR_MAX_LEN = 500, 100000
COMP = np.array([3, 2, 1, 0, 4, 5, 6, 7], np.uint8)  # CSeqTrans::ReverseComplement: a<->t, c<->g, the rest as it is


def new_stats(max_len, n_entries):
    return dict(q_insts=np.zeros((4, max_len), np.uint64), q_subs=np.zeros((4, max_len), np.uint64), m_sub=np.zeros(max_len + 1, np.uint64),
                max_align_len=0, n_accepted=0, ent_hits=np.zeros(n_entries, np.uint32), ent_uniq_loci=np.zeros(n_entries, np.uint32),
                ent_indeterminate=np.zeros(n_entries, np.uint32), ent_trimer=np.zeros((n_entries, 64), np.uint32))


def adj_start(r):
    return r["loci"] + (r["tl"] if r["strand"] == "+" else r["tr"])


def write_sub_dist(st, r, genome):
    """WriteSubDist: one reported read"""
    if r["nar"] != NAR_ACCEPTED or r["segs"] or r["chrom"] == 0:
        return
    hit_len = r["mlen"] - r["tl"] - r["tr"]  # AdjHitLen
    a0 = adj_start(r)
    assemb = genome[r["chrom"] - 1][a0:a0 + hit_len]  # GetSeq(ChromID, AdjStartLoci, AdjHitLen)
    if r["strand"] == "-":
        assemb = COMP[assemb[::-1]]
    read = r["read"]
    read_len = len(read)
    if st["max_align_len"] < read_len:
        st["max_align_len"] = read_len
    first = r["tl"]  # ReadOfs + TrimLeft, Seg[0].ReadOfs is 0
    last = read_len - r["tr"]
    seq = read[first:last]
    assert len(seq) == len(assemb), "a one-segment hit spans the read"
    band = (seq >> 6) & 3  # 4-bit score 0..3 -> 0, 4..7 -> 1, 8..11 -> 2, 12..15 -> 3
    idx = np.arange(first, last)
    differ = (seq & 7) != (assemb & 7)
    np.add.at(st["q_insts"], (band, idx), 1)
    np.add.at(st["q_subs"], (band[differ], idx[differ]), 1)
    st["m_sub"][int(differ.sum())] += 1


def targ_hit_counts(st, recs):
    """the counting of ReportTargHitCnts: the accepted reads in SortHitMatch order (chrom, AdjStartLoci, ...)"""
    acc = [r for r in recs if r["nar"] == NAR_ACCEPTED]
    acc.sort(key=lambda r: (r["chrom"], adj_start(r)))
    cur_targ, cur_loci, n_uniq = 0, None, 0
    for r in acc:
        if r["chrom"] != cur_targ:
            cur_targ, n_uniq = r["chrom"], 0
        e = cur_targ - 1
        tri, indet = 0, False
        for b in r["read"][:3]:
            b = int(b) & 7
            if b > 3:
                indet = True
                break
            tri = (tri << 2) | b
        if indet:
            st["ent_indeterminate"][e] += 1
        else:
            st["ent_trimer"][e, tri] += 1
        loci = adj_start(r)
        if n_uniq == 0 or loci != cur_loci:
            n_uniq += 1
            cur_loci = loci
            st["ent_uniq_loci"][e] += 1
        st["ent_hits"][e] += 1
    st["n_accepted"] = len(acc)


def collect(recs, genome, max_len, passes=1):
    """passes: 2 under `-A` with SAM output -- the splice junction file is open then (KAligner.cpp:4446), so WriteReadHits runs in
    front of WriteBAMReadHits (:745-757) and calls WriteSubDist for every read as well (:6835: eFMsam <= eFMbed)"""
    st = new_stats(max_len, len(genome))
    for _ in range(passes):
        for r in recs:
            write_sub_dist(st, r, genome)
    targ_hit_counts(st, recs)
    return st


def c_int(v):
    """what printf("%d") shows of a counter the reference keeps as int"""
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def main_text(st, ml_mode, max_multi, multi_hit):
    """WriteBasicCountStats; '' when nothing was accepted (KAligner.cpp:774)"""
    if not st["n_accepted"] or not st["max_align_len"]:
        return ""
    M = st["max_align_len"]
    o = []
    if ml_mode > 0:
        o.append('"Multihit distribution"\n,' + "".join(",%d" % (k + 1) for k in range(max_multi)))
        o.append('\n,,"Instances"' + "".join(",%d" % c_int(multi_hit[k]) for k in range(max_multi)) + "\n")
    psn = "".join(",%d" % (p + 1) for p in range(M))
    o.append('"Phred Score Instances"\n,"Psn"' + psn)
    for b, t in enumerate(("Phred 0..9", "Phred 10..19", "Phred 20..29", "Phred 30+")):
        o.append('\n,"%s"' % t + "".join(",%d" % c_int(v) for v in st["q_insts"][b, :M]))
    o.append('\n"Aligner Induced Subs"\n,"Psn"' + psn)
    for b, t in enumerate(("Phred 0..8", "Phred 9..19", "Phred 20..29", "Phred 30+")):
        o.append('\n,"%s"' % t + "".join(",%d" % c_int(v) for v in st["q_subs"][b, :M]))
    o.append('\n"Multiple substitutions"\n,"NumSubs"' + "".join(",%d" % p for p in range(M)))
    o.append('\n,"Instances"' + "".join(",%d" % c_int(v) for v in st["m_sub"][:M]) + "\n")
    return "".join(o)


def cnts_text(st, names, lens, n_reads):
    """ReportTargHitCnts' file; None when the reference writes none (KAligner.cpp:777)"""
    if not st["n_accepted"] or not st["max_align_len"]:
        return None
    o = ['"FeatID","TargSeq","TargLen","NumHits","RPKM","NumUniqueLoci"']
    o += [',"%s%s%s"' % ("ACGT"[(t >> 4) & 3], "ACGT"[(t >> 2) & 3], "ACGT"[t & 3]) for t in range(64)]
    o.append(",Indeterminates\n")
    with_hits = [e for e in range(len(names)) if st["ent_hits"][e]]
    last = with_hits[-1]
    for e in range(len(names)):
        nh = int(st["ent_hits"][e])
        if nh == 0:  # in front of a target with alignments "0.0" columns, behind the last one "0"
            o.append('%u,"%s",%u,0,0.0,0' % (e + 1, names[e], lens[e]) + (",0.0" if e < last else ",0") * 64 + ",0\n")
            continue
        rpkm = float(nh) * 1000.0
        rpkm /= float(lens[e])
        rpkm *= 1000000.0 / float(n_reads)
        o.append('%u,"%s",%u,%u,%f,%u' % (e + 1, names[e], lens[e], nh, rpkm, st["ent_uniq_loci"][e]))
        o.append("".join(",%1.4f" % (float(c) / float(nh)) for c in st["ent_trimer"][e]))
        o.append(",%u\n" % st["ent_indeterminate"][e])
    return "".join(o)


def peins_text(len_dist):
    return "".join("%d,%d\n" % (k, c_int(len_dist[k])) for k in range(PAIR_MAX_LEN + 1))


def multi_hit_dist(hit_rslt, inst):
    """m_MultiHitDist: LowHitInstances of the reads AlignRead takes as eHRhits (hit_rslt 1), as alignment leaves it"""
    d = np.zeros(MAX_MULTI, np.uint64)
    for h, i in zip(hit_rslt, inst):
        if h == 1 and i > 0:
            d[min(int(i), MAX_MULTI) - 1] += 1
    return d
