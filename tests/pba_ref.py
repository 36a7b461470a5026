"""`ngskit4b genpba` restated in plain Python / numpy, from SAM records and the genome: the per-locus pile-up of the accepted
alignments (CKAligner::ProcessSNPs, ngskit4b/KAligner.cpp:8168-8575), the packed-base-allele byte of every locus and the .pba file
(the PBA branch of OutputSNPs, :7194-7317) and the coverage WIG written beside it (AccumWIGCnts / CompleteWIGSpan, :6993-7085).

The restatement is pinned to the reference by tests/golden/make_golden_pba.py (it refuses to write a case this module does not
reproduce byte for byte) and by tests/test_pba_cpu.py."""
import re

import numpy as np

import samutil

# KAligner.h:124-129
PBA3, PBA2, PBA1 = 0.75, 0.35, 0.20
PBA2_LC, PBA1_LC = 0.70, 0.30
MAX_WIG_SPAN = 100000  # AccumWIGCnts' default MaxSpanLen

_CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")


def sam_alignments(recs, chrom_names):
    """(chromosome index, 0-based start, bases as read on the '+' strand) of every accepted alignment the pile-up takes: records
    with an indel or a splice junction in the CIGAR are skipped, soft clips are the alignment's trims; SEQ is already turned"""
    idx = {n: i for i, n in enumerate(chrom_names)}
    out = []
    for line in recs:
        f = line.split("\t")
        if int(f[1]) & 4 or f[2] == "*":
            continue
        ops = [(int(n), op) for n, op in _CIGAR.findall(f[5])]
        if any(op in "IDN" for _, op in ops):
            continue
        lead = ops[0][0] if ops[0][1] == "S" else 0
        trail = ops[-1][0] if len(ops) > 1 and ops[-1][1] == "S" else 0
        seq = f[9]
        bases = np.array([samutil.CODE.get(c, 4) for c in seq[lead:len(seq) - trail]], dtype=np.uint8)
        out.append((idx[f[2]], int(f[3]) - 1, bases))
    return out


def pileup(chroms, alns):
    """{chromosome index: uint32 [7, length]} -- NumRefBases, NumNonRefBases, NonRefBaseCnts[A, C, G, T, N] -- for every chromosome
    with at least one alignment that lies inside it.  A locus whose target base is N counts nothing; a read N counts into N and
    into the non-reference count."""
    cnts, stacks = {}, {}
    for c, start, bases in alns:
        if start + len(bases) > len(chroms[c]):  # GetSeq comes back short: the read is skipped (:8423)
            continue
        stacks.setdefault((c, start, len(bases)), []).append(bases)
    for (c, start, n), group in stacks.items():  # the reads of one span together: a column count per read base
        tgt = chroms[c]
        cnt = cnts.setdefault(c, np.zeros((7, len(tgt)), np.uint32))
        ref = tgt[start:start + n]
        rd = np.stack(group)
        for v in range(5):
            k = ((rd == v).sum(0) * (ref < 4)).astype(np.uint32)
            same = ref == v
            cnt[0, start:start + n] += np.where(same, k, 0).astype(np.uint32)
            cnt[1, start:start + n] += np.where(same, 0, k).astype(np.uint32)
            cnt[2 + v, start:start + n] += np.where(same, 0, k).astype(np.uint32)
    return cnts


def coverage(cnt7):
    return (cnt7[0] + cnt7[1] - cnt7[6]).astype(np.uint32)


def classify(cnt7, ref_bases):
    """the PBA byte per locus (:7262-7302): allele proportions as IEEE doubles against the reference's literals"""
    cov = coverage(cnt7)
    ref_bases = np.asarray(ref_bases)
    pba = np.zeros(cnt7.shape[1], np.uint8)
    covered = cov > 0
    div = np.where(covered, cov, 1).astype(np.float64)
    for b in range(4):
        n = np.where(ref_bases == b, cnt7[0], cnt7[2 + b])
        prop = n.astype(np.float64) / div
        hi = np.where(prop >= PBA3, 3, np.where(prop >= PBA2, 2, np.where(prop >= PBA1, 1, 0)))
        lo = np.where(prop >= PBA2_LC, 2, np.where(prop >= PBA1_LC, 1, 0))
        score = np.where(covered, np.where(cov >= 5, hi, lo), 0).astype(np.uint8)
        pba = ((pba << 2) | score).astype(np.uint8)
    return pba


def classify_locus(n_ref, n_non, by_base, ref_base):
    """one locus, with Python floats, line for line"""
    cov = n_non + n_ref - by_base[4]
    pba = 0
    if cov > 0:
        for b in range(4):
            pba <<= 2
            prop = (n_ref if b == ref_base else by_base[b]) / float(cov)
            if cov >= 5:
                if prop >= PBA3: pba |= 3
                elif prop >= PBA2: pba |= 2
                elif prop >= PBA1: pba |= 1
            else:
                if prop >= PBA2_LC: pba |= 2
                elif prop >= PBA1_LC: pba |= 1
    return pba, cov


def wig_chromosome(name, cov):
    """AccumWIGCnts over one chromosome with the locus counted from 1, between InitialiseWIGSpan and CompleteWIGSpan(true)"""
    out = []
    started, loci, length, cnts, rptd_len = False, 0, 0, 0, None

    def complete():
        nonlocal loci, length, cnts, rptd_len
        if started and length > 0 and loci > 0 and cnts > 0:
            if rptd_len != length:
                out.append("variableStep chrom=%s span=%d\n" % (name, length))
                rptd_len = length
            out.append("%d %d\n" % (loci, (cnts + length - 1) // length))
        loci = length = cnts = 0

    for l, c in enumerate(cov.tolist(), 1):
        if not started or length >= MAX_WIG_SPAN or c == 0:
            if started:
                complete()
            if c > 0:
                started, loci, length, cnts = True, l, 1, c
            continue
        if length == 0 or cnts == 0:
            loci, length, cnts = l, 1, c
            continue
        mean100 = 100 * (cnts // length)
        if (c <= 5 and c * 100 != mean100) or mean100 < c * 75 or mean100 >= c * 125:
            complete()
            loci, length, cnts = l, 1, c
            continue
        cnts += c
        length = l - loci + 1
    complete()
    return "".join(out)


def pba_files(names, chroms, alns, experiment_id, species, readset_id):
    """(the .pba file's bytes, the .covsegs.wig text, number of chromosome records, {chromosome index: (cnt7, pba, coverage)})"""
    cnts = pileup(chroms, alns)
    blob, wig, per = b"", [], {}
    for c in sorted(cnts):
        if not blob:
            blob = ("Type:PbA\nVersion:1\nExperimentID:%s\nReferenceID:%s\nReadsetID:%s" % (experiment_id, species, readset_id)).encode() + b"\0"
        pba, cov = classify(cnts[c], chroms[c]), coverage(cnts[c])
        nm = names[c].encode()
        blob += bytes([len(nm)]) + nm + b"\0" + len(chroms[c]).to_bytes(4, "little") + pba.tobytes()
        wig.append(wig_chromosome(names[c], cov))
        per[c] = (cnts[c], pba, cov)
    return blob, "".join(wig), len(cnts), per


def parse_pba(blob):
    """(header text, [(name, bytes as uint8 array)]) of a .pba file"""
    if not blob:
        return "", []
    end = blob.index(b"\0")
    hdr, at, recs = blob[:end].decode(), end + 1, []
    while at < len(blob):
        nl = blob[at]
        name = blob[at + 1:at + 1 + nl].decode()
        assert blob[at + 1 + nl] == 0
        n = int.from_bytes(blob[at + 2 + nl:at + 6 + nl], "little")
        recs.append((name, np.frombuffer(blob, np.uint8, n, at + 6 + nl)))
        at += 6 + nl + n
    return hdr, recs
