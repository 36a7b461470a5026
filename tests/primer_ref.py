"""A literal Python restatement of kalign's 5' PCR primer correction (`-6 <n>`): CKAligner::PCR5PrimerCorrect,
ngskit4b/KAligner.cpp:2115-2226, as CKAligner::Align calls it (:642-651) with the user's MaxSubs behind ReducePCRduplicates and in
front of AutoTrimFlanks, over reads aligned with min(MaxSubs + n, 15) substitutions per 100 bp (:245-248).  It checks the device
stage (kit4b_amd/csrc/k4_primer.hip) and the golden runs (tests/golden/make_golden_primer.py).

A record is a dict: nar, num_hits, two_seg (HitLoci.FlagSegs), match_len / loci / chrom (1-based) / strand ('+' | '-') of Seg[0],
read_len, low_mm (LowMMCnt), mismatches (Seg[0].Mismatches) and seq, a mutable sequence of the read's bytes as loaded (symbol in
bits 0..2, the quality score above).  target(chrom, loci, n) is CSfxArray::GetSeq: n symbols of the sequence from loci.
"""
import numpy as np

NAR_ACCEPTED, NAR_NOHIT = 1, 3
KLEN = 12  # the KLen default (KAligner.h:850); kalign passes no other
MAX_ALLOWED_SUBS = 15  # cMaxAllowedSubs, KAligner.h:37
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
LETTER = "ACGTN"


def initial_align_subs(max_subs, primer_subs):
    """m_InitalAlignSubs (:245-248): what LocateCoredApprox and ProcessPairedEnds are given"""
    return min(max_subs + primer_subs, MAX_ALLOWED_SUBS) if primer_subs > 0 else max_subs


def reverse_complement(seq):
    """CSeqTrans::ReverseComplement (libkit4b/SeqTrans.cpp:497-551): A<->T, C<->G, every other symbol as it is"""
    return [3 - b if b <= 3 else b for b in reversed(seq)]


def pcr5_primer_correct(recs, max_allowed_sub_rate, target, klen=KLEN):
    """the walk over all reads; returns [reads corrected, bases corrected, reads rejected]"""
    n_reads = n_bases = n_rejected = 0
    if klen < 1:
        return [0, 0, 0]
    for r in recs:
        if r["nar"] != NAR_ACCEPTED or r["two_seg"]:
            continue
        max_mms = (max_allowed_sub_rate * r["read_len"] + 50) // 100
        if r["low_mm"] <= max_mms:  # already meeting the targeted rate
            continue
        match_len = r["match_len"]
        if match_len != r["read_len"]:
            continue
        targ = list(target(r["chrom"], r["loci"], match_len))
        if r["strand"] == "-":
            targ = reverse_complement(targ)
        seq = r["seq"]
        cur = r["low_mm"]
        for ofs in range(klen):
            if (seq[ofs] & 0x07) != targ[ofs]:
                cur -= 1
                if cur <= max_mms:
                    break
        if cur <= max_mms:
            cur = r["low_mm"]
            for ofs in range(klen):
                base = seq[ofs]
                if (base & 0x07) != targ[ofs]:
                    seq[ofs] = (base & 0xF8) | targ[ofs]
                    n_bases += 1
                    cur -= 1
                    if cur <= max_mms:
                        break
            r["low_mm"] = r["mismatches"] = cur
            n_reads += 1
        else:
            r["num_hits"] = 0
            r["nar"] = NAR_NOHIT
            n_rejected += 1
    return [n_reads, n_bases, n_rejected]


# ---- over a -M1 SAM of the run without -6 (tests/golden/primer_base_*.sam.xz) ----------------------------------------------------
def sam_records(lines, names, chroms):
    """one record per SAM line, in file order.  key: QNAME/<0 | 1: second in pair>.  The SAM shows an accepted read in the target's
    sense: seq is turned back to the read as loaded.  LowMMCnt of a one-segment full-length alignment is its Hamming distance."""
    recs = []
    for line in lines:
        f = line.split("\t")
        flag = int(f[1])
        r = dict(key=f[0] + "/" + str((flag >> 7) & 1), line=line, nar=NAR_ACCEPTED, num_hits=1, two_seg=False, read_len=len(f[9]))
        if "YU:Z:" in line:
            r["nar"] = -1  # (some other NAR: the stage passes over it)
            r["code"] = line.rsplit("YU:Z:", 1)[1].strip()
            r["seq"] = [CODE[c] for c in f[9]]
            recs.append(r)
            continue
        minus = bool(flag & 16)
        shown = [CODE[c] for c in f[9]]
        r["seq"] = reverse_complement(shown) if minus else shown
        cigar = f[5]
        r["two_seg"] = any(c in cigar for c in "NID")
        r["clipped"] = "S" in cigar
        r["chrom"], r["loci"], r["strand"] = names.index(f[2]) + 1, int(f[3]) - 1, "-" if minus else "+"
        r["match_len"] = int(cigar[:-1]) if cigar[:-1].isdigit() else 0
        if not r["two_seg"] and not r["clipped"]:
            t = chroms[r["chrom"] - 1][r["loci"]:r["loci"] + r["match_len"]]
            r["low_mm"] = r["mismatches"] = sum(1 for a, b in zip(shown, t) if a != int(b))
        else:
            r["low_mm"] = r["mismatches"] = 0
        recs.append(r)
    return recs


def genome_target(chroms):
    arrays = [np.asarray(c, np.uint8) for c in chroms]
    return lambda chrom, loci, n: arrays[chrom - 1][loci:loci + n].tolist()


def sam_seq(r):
    """SEQ as the SAM shows the record now"""
    s = reverse_complement(r["seq"]) if r["nar"] == NAR_ACCEPTED and r["strand"] == "-" else r["seq"]
    return "".join(LETTER[b & 7] for b in s)


def sam_line(r):
    """the record's line with its SEQ as it is now"""
    f = r["line"].split("\t")
    f[9] = sam_seq(r)
    return "\t".join(f)
