"""kalign's SNP centroids (-7) and marker sequences (-K) restated in plain Python, from SAM records and the genome: the pile-up of
tests/pba_ref.py, then OutputSNPs' locus loop (ngskit4b/KAligner.cpp:7320-7579) up to the marker gate -- centroid instance counts,
the candidate tests, the background window and noise test, the marker walk -- and the centroid file (:8104-8133, :8626-8660).
The p-values and the Benjamini-Hochberg cut are NOT restated: the called loci are read from a SNP file (CSV or VCF).

Pinned to the reference by tests/test_markers_cpu.py (every golden centroid and markers file, byte for byte)."""
import numpy as np

FLANK, CENT_LEN, CENT_BINS = 3, 7, 16384  # cSNPCentfFlankLen, cSNPCentroidLen, cSNPCentroidEls
WIN_FLANK = 25                             # cSNPBkgndRateWindow / 2
MIN_ERR_RATE, MAX_NOISE = 0.005, 0.20      # cMinSeqErrRate, cMaxBkgdNoiseThres
DFLT_POLY_THRES = 1.0 / 3.0                # cDfltMinMarkerSNPProp
ASCII = "ACGTN"


def centroid_index(tgt, l):
    """index of the reference 7-mer around locus l (first base in the highest bits), or None: too close to an end / a non-ACGT symbol"""
    if l < FLANK or l >= len(tgt) - FLANK:
        return None
    idx = 0
    for b in tgt[l - FLANK:l + FLANK + 1]:
        if b > 3:
            return None
        idx = (idx << 2) | int(b)
    return idx


def marker_locus(n_ref, n_non, by_base, ref_base, min_snp_reads, poly_thres):
    """one marker locus (:7515-7535), with Python floats, line for line: (base 0..4 | 'coverage' | 'allele', polymorphic)"""
    tot = n_non + n_ref
    if tot < min_snp_reads:
        return "coverage", False
    prop = float(n_non) / tot
    if prop <= poly_thres:
        return min(int(ref_base), 4), prop > 0.1
    for b in range(5):
        if by_base[b] > 0:
            prop = float(by_base[b]) / tot
            if prop >= (1.0 - poly_thres):
                return b, prop < 0.9
    return "allele", False


def marker_at(cnt7, tgt, l, marker_len, min_snp_reads, poly_thres):
    """the marker gate for the candidate at locus l (:7497-7545): (sequence, polymorphic sites) or (None, why)"""
    m5 = marker_len // 2
    m3 = marker_len - 1 - m5
    if l < m5:
        return None, "start"
    if l + m3 >= len(tgt):
        return None, "end"
    tot = int(cnt7[0, l]) + int(cnt7[1, l])
    if float(cnt7[1, l]) / tot < 0.5:
        return None, "proportion"
    seq, poly = [], 0
    for ml in range(l - m5, l - m5 + marker_len):
        b, p = marker_locus(int(cnt7[0, ml]), int(cnt7[1, ml]), [int(x) for x in cnt7[2:7, ml]], tgt[ml], min_snp_reads, poly_thres)
        if isinstance(b, str):
            return None, b
        seq.append(ASCII[b])
        poly += p
    if seq[m5] == ASCII[min(int(tgt[l]), 4)]:
        return None, "centre"
    return "".join(seq), poly


def chromosome(cnt7, tgt, min_snp_reads, nonref_pcnt):
    """the locus loop of one chromosome up to the noise test: (loci counted for the centroids, candidate loci that pass the noise test)"""
    clen = len(tgt)
    n_ref, n_non = cnt7[0].astype(np.int64), cnt7[1].astype(np.int64)
    tot = n_ref + n_non
    glob = max(MIN_ERR_RATE, float(n_non.sum()) / float(1 + n_ref.sum() + n_non.sum()))
    win = 2 * WIN_FLANK + 1
    # the sliding sums: the first `win` loci, moved one locus for every locus in (flank, clen - flank)
    lo = np.zeros(clen, np.int64)
    if clen > win:
        l = np.arange(clen)
        lo = np.where(l <= WIN_FLANK, 0, np.where(l + WIN_FLANK < clen, l - WIN_FLANK, clen - win))
    hi = np.minimum(lo + win, clen)
    p_ref, p_non = np.concatenate([[0], np.cumsum(n_ref)]), np.concatenate([[0], np.cumsum(n_non)])
    loc_m, loc_mm = p_ref[hi] - p_ref[lo], p_non[hi] - p_non[lo]
    deep = np.flatnonzero(tot >= min_snp_reads)
    frac = nonref_pcnt / 100.0
    survivors = []
    for l in deep.tolist():
        if n_non[l] < 1 or float(n_non[l]) / float(tot[l]) < frac:
            continue
        tmm = int(loc_mm[l] - n_non[l]) if n_non[l] <= loc_mm[l] else 0
        tm = int(loc_m[l] - n_ref[l]) if n_ref[l] < loc_m[l] else 0
        rate = glob if tmm + tm == 0 else max(float(tmm) / float(tmm + tm), glob)
        if rate > MAX_NOISE:
            continue
        survivors.append(l)
    return deep.tolist(), survivors


def sliding_window_sums(n_ref, n_non):
    """the reference's own loop (:7330-7366), locus by locus: what `chromosome` computes from prefix sums"""
    clen, win = len(n_ref), 2 * WIN_FLANK + 1
    m, mm = int(sum(n_ref[:win])), int(sum(n_non[:win]))
    left, right, out = 0, min(win, clen), []
    for l in range(clen):
        if l > WIN_FLANK and l + WIN_FLANK < clen:
            mm = mm - int(n_non[left]) if mm >= n_non[left] else 0
            m = m - int(n_ref[left]) if m >= n_ref[left] else 0
            mm += int(n_non[right])
            m += int(n_ref[right])
            left += 1
            right += 1
        out.append((m, mm))
    return out


def run(names, chroms, cnts, min_snp_reads=5, nonref_pcnt=25.0, marker_len=0, poly_thres=DFLT_POLY_THRES):
    """the whole run: {"insts": NumInsts per 7-mer, "survivors": {chromosome: loci that reach the p-value}, "markers": the .markers
    text, "ids": {(chromosome, locus): (MarkerID, NumPolymorphicSites)}, "rejects": {why: count}}"""
    insts = np.zeros(CENT_BINS, np.int64)
    out = {"survivors": {}, "markers": [], "ids": {}, "rejects": {}}
    marker_id = 0
    for c in sorted(cnts):
        tgt, cnt7 = chroms[c], cnts[c]
        deep, surv = chromosome(cnt7, tgt, min_snp_reads, nonref_pcnt)
        for l in deep:
            idx = centroid_index(tgt, l)
            if idx is not None:
                insts[idx] += 1
        if marker_len:
            kept = []
            for l in surv:
                seq, poly = marker_at(cnt7, tgt, l, marker_len, min_snp_reads, poly_thres)
                if seq is None:
                    out["rejects"][poly] = out["rejects"].get(poly, 0) + 1
                    continue
                marker_id += 1
                m5 = marker_len // 2
                out["markers"].append(">Marker%d %s %d|%d|%d|%d|%s|%s|%d\n%s\n" % (marker_id, names[c], l - m5, marker_len, l, m5, seq[m5],
                                                                                 ASCII[min(int(tgt[l]), 4)], poly, seq))
                out["ids"][(c, l)] = (marker_id, poly)
                kept.append(l)
            surv = kept
        out["survivors"][c] = surv
    out["insts"] = insts
    out["markers"] = "".join(out["markers"])
    out["n_markers"] = marker_id
    return out


def called_loci(snp_text, names):
    """[(chromosome index, locus)] of a SNP file, CSV or VCF, in file order; for the CSV also {(chromosome, locus): (MarkerID, NumPolymorphicSites)}"""
    idx = {n: i for i, n in enumerate(names)}
    loci, cols = [], {}
    for line in snp_text.splitlines():
        if line.startswith("#") or line.startswith('"SNP_ID"'):
            continue
        if "\t" in line:
            f = line.split("\t")
            loci.append((idx[f[0]], int(f[1]) - 1))
        else:
            f = line.split(",")
            key = (idx[f[3].strip('"')], int(f[4]))
            loci.append(key)
            cols[key] = (int(f[21]), int(f[22]))
    return loci, cols


def centroid_text(insts, chroms, cnts, called):
    """the centroid file: NumInsts from `run`, the SNP columns from the called loci's counts as piled"""
    rows = np.zeros((CENT_BINS, 7), np.int64)  # NumSNPs, RefBaseCnt, A, C, G, T, N
    for c, l in called:
        idx = centroid_index(chroms[c], l)
        if idx is None:
            continue
        rows[idx, 0] += 1
        rows[idx, 1] += int(cnts[c][0, l])
        rows[idx, 2:7] += cnts[c][2:7, l].astype(np.int64)
    out = ['"CentroidID","Seq","NumInsts","NumSNPs","RefBase","RefBaseCnt","BaseA","BaseC","BaseG","BaseT","BaseN"\n']
    for i in range(CENT_BINS):
        seq = "".join("ACGT"[(i >> (2 * (6 - k))) & 3] for k in range(CENT_LEN))
        r = rows[i]
        out.append('%d,"%s",%d,%d,"%s",%d,%d,%d,%d,%d,%d\n' % (i + 1, seq, insts[i], r[0], seq[FLANK], r[1], r[2], r[3], r[4], r[5], r[6]))
    return "".join(out)
