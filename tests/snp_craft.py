"""Crafted inputs of the SNP calling stage (k4_snp_run_dev: pile-up, candidate kernel, haplotype kernel, coverage for the WIG): small
genomes of their own with alignments laid out directly -- strand, trims, `ext` word and NAR chosen per alignment -- at the chromosome
ends of the 51-base background window, at the equalities of the candidate tests, at the read ends and separations the haplotype files
turn on, at the 1 / 2 / 4 byte coverage forms and around the WIG's bookkeeping.  tests/test_snp_craft_cpu.py checks on the oracle and
the plain pile-up that they hold what they are built for; tests/test_gpu_snp_crafted.py runs the device against the oracle on them.

A scenario is dict(chroms, alns, opts, pe, vcf, expect): `alns` are lists [sequence, start of the whole read on the sequence, the
whole read's bases as they lie on the '+' strand, minus, TrimLeft, TrimRight, flags of the ext word, NAR]; `opts` the option sets it
is meant for; `expect` what it was built to contain (per option set where that differs)."""
import functools
import math

import numpy as np

import markers_ref
import synth
from oracle_bindings import EXT_CHIMERIC, EXT_INDEL, EXT_NONORPHAN, EXT_SPLICE, HIT_DTYPE, PE_READ_DTYPE, RESULT_DTYPE
from test_gpu_markers import other, put, tile

DFLT = dict(min_snp_reads=5, qvalue=0.05, snp_nonref_pcnt=25.0)


def names_of(chroms):
    return ["m%02d" % i for i in range(len(chroms))]  # (as test_gpu_markers.build_index names them)


def aln(c, start, fwd, minus=False, tl=0, tr=0, flags=0, nar=1):
    return [c, start, np.array(fwd, np.uint8), bool(minus), tl, tr, flags, nar]


def tiled(c, tgt, depth, **kw):
    """tile()'s layers as alignments, every other one on the '-' strand"""
    return [aln(a[0], a[1], a[2], i & 1) for i, a in enumerate(tile(c, tgt, depth, **kw))]


def stack(c, tgt, lo, hi, haps, loci, lead=0, trail=0, flags=0, first_minus=0):
    """len(haps) reads over tgt[lo..hi], the j-th on strand (j + first_minus) & 1.  haps[j] says what read j shows at those of the
    called `loci` it spans, in their order: R the reference base, A the alternative one (other()), N.  lead / trail: bases trimmed
    at the low / high end of the span (TrimLeft / TrimRight by the read's strand); what lies in a trimmed flank mismatches everywhere."""
    inside = [l for l in loci if lo <= l <= hi]
    out = []
    for j, hap in enumerate(haps):
        assert len(hap) == len(inside), (lo, hi, hap, inside)
        fwd = tgt[lo:hi + 1].copy()
        for l, h in zip(inside, hap):
            fwd[l - lo] = {"R": tgt[l], "A": other(tgt[l]), "N": 4}[h]
        n = len(fwd)
        for q in list(range(lead)) + list(range(n - trail, n)):
            fwd[q] = other(tgt[lo + q], 2)
        minus = bool((j + first_minus) & 1)
        tl, tr = (trail, lead) if minus else (lead, trail)  # the trims count from the read's own ends
        out.append(aln(c, lo, fwd, minus, tl, tr, flags))
    return out


def materialise(alns):
    """(reads, results, hits) as the device and the oracle take them, and the (sequence, start, '+' strand bases) list of the
    alignments a pile-up takes, for pba_ref.pileup (which leaves out by itself what reaches over a sequence's end)"""
    n = len(alns)
    hits, rr = np.zeros(n, HIT_DTYPE), np.zeros(n, RESULT_DTYPE)
    reads, piled = [], []
    for i, (c, start, fwd, minus, tl, tr, flags, nar) in enumerate(alns):
        reads.append(synth.revcomp(fwd) if minus else fwd)
        hits[i] = (c + 1, start, len(fwd), ord("-") if minus else ord("+"), 0, tl | (tr << 12) | flags)
        rr[i] = (1, 1 if nar == 1 else 0, 0, 1, nar, 1 if nar == 1 else 0)
        if nar == 1 and not flags & (EXT_INDEL | EXT_SPLICE):
            lead, trail = (tr, tl) if minus else (tl, tr)
            piled.append((c, start + lead, fwd[lead:len(fwd) - trail]))
    return reads, rr, hits, piled


def as_pe(reads, rr, hits):
    """the same alignments as PE records with interleaved reads (an odd number: one read without an alignment is added)"""
    reads = list(reads)
    if len(reads) & 1:
        reads.append(np.zeros(30, np.uint8))
        rr = np.concatenate([rr, np.zeros(1, RESULT_DTYPE)])
        rr[-1]["nar"] = 3
        hits = np.concatenate([hits, np.zeros(1, HIT_DTYPE)])
    pe = np.zeros(len(rr), PE_READ_DTYPE)
    for k in ("nar", "num_hits", "inst", "low_mm"):
        pe[k] = rr[k]
    pe["pe_aligned"] = rr["nar"] == 1
    pe["hit"] = hits
    return reads, pe


# ---- reading the files back ----------------------------------------------------------------------------------------------------
def called(snp_text):
    """{sequence name: [locus]} of a SNP file, CSV or VCF records"""
    out = {}
    for ln in snp_text.splitlines():
        if ln.startswith(("#", '"SNP_ID"')):
            continue
        f = ln.split("\t") if "\t" in ln else None
        name, l = (f[0], int(f[1]) - 1) if f else (ln.split(",")[3].strip('"'), int(ln.split(",")[4]))
        out.setdefault(name, []).append(l)
    return out


def csv_rows(snp_text):
    """{(sequence name, locus): the CSV row's fields}"""
    out = {}
    for ln in snp_text.splitlines()[1:]:
        f = ln.split(",")
        out[(f[3].strip('"'), int(f[4]))] = f
    return out


def wig_spans(text):
    """{sequence name: [(first locus, span length, value)]} of a .covsegs.wig"""
    out, name, span = {}, None, 0
    for ln in text.splitlines()[1:]:
        if ln.startswith("variableStep"):
            f = dict(x.split("=") for x in ln.split()[1:])
            name, span = f["chrom"], int(f["span"])
        else:
            l, v = ln.split()
            out.setdefault(name, []).append((int(l), span, int(v)))
    return out


def hap_lines(text):
    """[(sequence name, (loci...), depth, antisense, haplotypes)] of a .disnp.csv / .trisnp.csv"""
    out = []
    n = 2 if text.startswith('"DiSNPs') else 3
    for ln in text.splitlines()[1:]:
        f = ln.split(",")
        out.append((f[3].strip('"'), tuple(int(f[4 + 7 * k]) for k in range(n)), int(f[4 + 7 * n]), int(f[5 + 7 * n]), int(f[6 + 7 * n])))
    return out


def why_not(cnt7, l, opts):
    """which of OutputSNPs' tests (KAligner.cpp:7375-7450) stops locus l, from the plain pile-up and the reference's own sliding
    sums: 'coverage', 'reference' (no mismatch), 'proportion', 'noise'; None = it reaches the p-value (so only the cut can drop it)"""
    n_ref, n_non = cnt7[0].astype(np.int64), cnt7[1].astype(np.int64)
    tot = int(n_ref[l] + n_non[l])
    if tot < opts["min_snp_reads"]:
        return "coverage"
    if n_non[l] < 1:
        return "reference"
    if float(n_non[l]) / tot < opts["snp_nonref_pcnt"] / 100.0:
        return "proportion"
    m, mm = markers_ref.sliding_window_sums(n_ref.tolist(), n_non.tolist())[l]
    tmm = mm - int(n_non[l]) if n_non[l] <= mm else 0
    tm = m - int(n_ref[l]) if n_ref[l] < m else 0
    glob = max(markers_ref.MIN_ERR_RATE, float(n_non.sum()) / float(1 + n_ref.sum() + n_non.sum()))
    rate = glob if tmm + tm == 0 else max(float(tmm) / float(tmm + tm), glob)
    return "noise" if rate > markers_ref.MAX_NOISE else None


# ---- (a) windows -----------------------------------------------------------------------------------------------------------------
WINDOW_LENS = [1, 25, 50, 51, 52, 77, 255, 256, 257, 1000]


def windows():
    """(a) homozygous SNPs at depth 8 at both ends of the background window's clamping, on sequences of 1, 25, 50, 51, 52 and 77
    bases (loci 0, clen - 1, 24, 25, 26, clen - 27, clen - 26, clen - 25 where they exist) and of 255, 256, 257 and 1000 bases (0, 25,
    26, 255, 256, clen - 27, clen - 26, clen - 25, clen - 1).  Loci 51 and clen - 52 -- the ones the window takes up / lets go when it
    first / last moves -- are covered by six reads where the sequence's two end loci have eight, so TotWinBases differs between
    loci 25 and 26 and between clen - 27 and clen - 26 (on the 52-base sequence locus 51 is itself the last SNP: six reads there).
    About one other locus in nine has six reads too and about one in fifteen one substituted read.  m10 has a reference N run of 60
    bases with a SNP on either side, m11 no read.
    Ends up with: 64 called loci; m00's only locus is a candidate and falls to the noise test (nothing but itself in its window: the
    sequence's own mismatch rate, 8 / 9, is its background)."""
    rng = np.random.default_rng(0x51A0)
    chroms = [rng.integers(0, 4, n).astype(np.uint8) for n in WINDOW_LENS + [400, 300]]
    chroms[10][170:230] = 4
    snps = {}
    for c, clen in enumerate(WINDOW_LENS):
        want = {0, clen - 1, 24, 25, 26, clen - 27, clen - 26, clen - 25} | ({255, 256} if clen >= 255 else set())
        snps[c] = sorted(l for l in want if 0 <= l < clen)
    snps[10] = [169, 230]
    alns = []
    for c in range(11):
        clen = len(chroms[c])
        edge = {51} if clen == 52 else {l for l in (51, clen - 52) if clen > 52}
        free = [l for l in range(clen) if l not in snps[c] and l not in edge and chroms[c][l] < 4]
        pick = rng.random(len(free))
        part = tiled(c, chroms[c], 8, holes=sorted(edge | {l for l, p in zip(free, pick) if p < 1 / 9}))
        for l in snps[c]:
            put(part, c, l, other(chroms[c][l]))
        for l, p in zip(free, pick):
            if 1 / 9 <= p < 1 / 9 + 1 / 15:
                put(part, c, l, other(chroms[c][l], 2), 1)
        alns += part
    expect = dict(called={c: (snps[c] if c else []) for c in range(11)}, absent={(0, 0): "noise"},
                  edges=[(c, a, b) for c, clen in enumerate(WINDOW_LENS) if clen > 51 for a, b in ((25, 26), (clen - 27, clen - 26))])
    return dict(chroms=chroms, alns=alns, opts=[DFLT], expect=[expect])


# ---- (b) thresholds, (g) vcf ---------------------------------------------------------------------------------------------------------
TINY_Q = dict(DFLT, qvalue=1e-9)


def thresholds():
    """(b) m00, eight reads deep over [0, 1400), five over [1500, 1600), four over [1700, 1800):
      40, 300       all eight reads show N (40 is the run's first called SNP; 300 follows the ordinary SNP at 200)
      100           2 of 8: (double)2 / 8 < 0.25 is false, a candidate
      200           an ordinary homozygous SNP
      594..605      twelve homozygous SNPs side by side: each has 88 mismatches among the 400 other bases of its window, 0.22: noise
      896..905      ten of them with seven single substitutions at 880..886: 79 of 400, 0.1975, they stay
      1150          2 of 8 with one substituted read at each of the 50 other loci of its window: background 0.125, p = 0.067
      1520, 1550    1 of 5 (proportion) and 5 of 5 at coverage min_snp_reads; 1750: 4 of 4 at coverage min_snp_reads - 1
    m01, eight deep from locus 10 on (one WIG span, closed at the sequence's end only): 2 of 8 at 100, 300 and 500, nothing else; their
    p-values are about 7e-6.
    Ends up with: q 0.05 calls 15 loci of m00 (1150 falls to the cut: its p-value is the largest, so it faces q itself) and m01's
    three; q 1e-9 calls the 14 of m00 whose p-value is 0 and none of m01, whose candidates still close the WIG's last span."""
    rng = np.random.default_rng(0x7B0)
    chroms = [rng.integers(0, 4, 2400).astype(np.uint8), rng.integers(0, 4, 600).astype(np.uint8)]
    t = chroms[0]
    alns = tiled(0, t, 8, last=1400) + tiled(0, t, 5, first=1500, last=1600) + tiled(0, t, 4, first=1700, last=1800) + tiled(1, chroms[1], 8, first=10)
    for l in (40, 300):
        put(alns, 0, l, 4)
    for l in [200, 1550, 1750] + list(range(594, 606)) + list(range(896, 906)):
        put(alns, 0, l, other(t[l]))
    for l in (100, 1150):
        put(alns, 0, l, other(t[l]), 2)
    for l in list(range(880, 887)) + [l for l in range(1125, 1176) if l != 1150] + [1520]:
        put(alns, 0, l, other(t[l], 2), 1)
    for l in (100, 300, 500):
        put(alns, 1, l, other(chroms[1][l]), 2)
    zero_p = [40, 200, 300] + list(range(896, 906)) + [1550]
    absent = {(0, l): "noise" for l in range(594, 606)}
    absent.update({(0, 1150): "cut", (0, 1520): "proportion", (0, 1750): "coverage", (0, 885): "proportion"})
    e1 = dict(called={0: sorted(zero_p + [100]), 1: [100, 300, 500]}, absent=absent)
    e2 = dict(called={0: sorted(zero_p), 1: []}, absent={**absent, (0, 100): "cut", (1, 100): "cut", (1, 300): "cut", (1, 500): "cut"})
    return dict(chroms=chroms, alns=alns, opts=[DFLT, TINY_Q], expect=[e1, e2])


def vcf():
    """(g) the sequences of (b) in the VCF form: the run's first record (m00 locus 40) has only N mismatches, so ALT and AF are empty;
    the record of locus 300, N only too, repeats the ALT and AF strings the SNP at 200 left behind"""
    s = thresholds()
    return dict(s, opts=[DFLT], expect=[s["expect"][0]], vcf=True)


# ---- (c) haplotypes, (f) pe_form --------------------------------------------------------------------------------------------------
HAP_MAX_SEP = 58
H3 = ["AAA"] * 6 + ["RRR"] * 6 + ["ARA"] * 6


def haplotypes():
    """(c) m00 (mean aligned length between 57 and 58: pairs up to 58 apart), its called loci in groups more than 58 apart:
      300, 320             6 + 6 reads over both; one read of either strand that starts at 300, ends at 320, ends at 319, starts at 301
      600, 615, 630        6 + 6 + 6 reads over all three (AAA, RRR, ARA); three over the first two only, three over the last two only;
                           one read of either strand with N at the first, at the middle, at the last locus
      900 .. 940 by 10     a run of five under AAAAA, RRRRR and ARARA: the triple ending at locus k shows the base of k - 2, not of k - 3
      1200, 1215           AA x 5, RR x 5, AR x 4: threshold 5, AR stays one below (it prints as 0)
      1350, 1365           AA x 30, RR x 22, AR x 7, RA x 6: depth 65, threshold (65 + 5) / 10 = 7, RA stays one below
      1500, 1515           AA x 10 alone: one haplotype, no line
      1800, 1830           ten reads over each alone, four over both: min_snp_reads - 1, no line
      2100, 2158           58 apart, a line;   2400, 2459: 59 apart, none, though twelve reads span them
      2700, 2720, 2740     AAA, RRR, ARA, and reads flagged chimeric on either strand whose trimmed low end takes 2700 with it / ends
                           one base before it, whose trimmed high end starts one base behind 2740 / takes it along, and both
    m01: called loci 0, 5 and 9.  m02: 400-base reads, max_sep 300: 500 and 800, a line; 1500 and 1801, none.  m03: one called
    locus.  m04: two.  (No read shows N at a called locus behind the group at 600.)
    Ends up with: 35 called loci; 16 DiSNP lines (m00 12, m01 2, m02 1, m04 1) and 6 TriSNP lines (m00 5, m01 1)."""
    rng = np.random.default_rng(0xC0DE)
    chroms = [rng.integers(0, 4, n).astype(np.uint8) for n in (4000, 300, 3000, 300, 300)]
    t = chroms[0]
    loci = [300, 320, 600, 615, 630, 900, 910, 920, 930, 940, 1200, 1215, 1350, 1365, 1500, 1515, 1800, 1830, 2100, 2158, 2400, 2459, 2700, 2720, 2740]
    a = stack(0, t, 280, 340, ["AA"] * 6 + ["RR"] * 6, loci)
    for fm in (0, 1):
        a += stack(0, t, 300, 340, ["AA"], loci, first_minus=fm) + stack(0, t, 280, 320, ["RR"], loci, first_minus=fm)
        a += stack(0, t, 280, 319, ["A"], loci, first_minus=fm) + stack(0, t, 301, 340, ["R"], loci, first_minus=fm)
    a += stack(0, t, 580, 650, H3, loci) + stack(0, t, 580, 620, ["AA", "RR", "AR"], loci) + stack(0, t, 610, 650, ["AA", "RR", "RA"], loci, first_minus=1)
    a += stack(0, t, 580, 650, ["NAA", "NRR", "ANA", "RNR", "AAN", "RRN"], loci)
    a += stack(0, t, 880, 960, ["AAAAA"] * 6 + ["RRRRR"] * 6 + ["ARARA"] * 6, loci)
    a += stack(0, t, 1185, 1230, ["AA"] * 5 + ["RR"] * 5 + ["AR"] * 4, loci)
    a += stack(0, t, 1335, 1380, ["AA"] * 30 + ["RR"] * 22 + ["AR"] * 7 + ["RA"] * 6, loci)
    a += stack(0, t, 1485, 1530, ["AA"] * 10, loci)
    a += stack(0, t, 1780, 1815, ["A", "R"] * 5, loci) + stack(0, t, 1816, 1850, ["A", "R"] * 5, loci) + stack(0, t, 1790, 1840, ["AA", "AA", "RR", "RR"], loci)
    a += stack(0, t, 2090, 2170, ["AA"] * 6 + ["RR"] * 6, loci) + stack(0, t, 2390, 2470, ["AA"] * 6 + ["RR"] * 6, loci)
    a += stack(0, t, 2680, 2760, H3, loci)
    for lead, trail, hap in ((21, 0, "AAA"), (20, 0, "AAA"), (0, 20, "AAA"), (0, 21, "AAA"), (21, 21, "RRR")):
        for fm in (0, 1):  # (stack() writes the haplotype first and the mismatching flanks over it)
            a += stack(0, t, 2680, 2760, [hap], loci, lead=lead, trail=trail, flags=EXT_CHIMERIC, first_minus=fm)
    # reads far from every called locus that bring the mean aligned length between 57 and 58
    tot, n = sum(len(x[2]) - x[4] - x[5] for x in a), len(a)
    while not HAP_MAX_SEP - 0.8 < tot / n < HAP_MAX_SEP - 0.2:
        ln = 20 if tot / n > HAP_MAX_SEP - 0.5 else 100
        a.append(aln(0, 3200 + (7 * n) % 600, t[3200 + (7 * n) % 600:][:ln], n & 1))
        tot, n = tot + ln, n + 1
    assert math.ceil(tot / n) == HAP_MAX_SEP and tot % n, (tot, n)
    a += stack(1, chroms[1], 0, 40, H3, [0, 5, 9])
    a += stack(2, chroms[2], 450, 849, ["AA"] * 6 + ["RR"] * 6, [500, 800]) + stack(2, chroms[2], 1450, 1849, ["AA"] * 6 + ["RR"] * 6, [1500, 1801])
    a += stack(3, chroms[3], 120, 180, ["A", "R"] * 5, [150])
    a += stack(4, chroms[4], 80, 150, ["AA"] * 6 + ["RR"] * 6, [100, 130])
    di = {0: [(300, 320), (600, 615), (615, 630), (900, 910), (910, 920), (920, 930), (930, 940), (1200, 1215), (1350, 1365), (2100, 2158), (2700, 2720),
              (2720, 2740)], 1: [(0, 5), (5, 9)], 2: [(500, 800)], 4: [(100, 130)]}
    tri = {0: [(600, 615, 630), (900, 910, 920), (910, 920, 930), (920, 930, 940), (2700, 2720, 2740)], 1: [(0, 5, 9)]}
    expect = dict(called={0: loci, 1: [0, 5, 9], 2: [500, 800, 1500, 1801], 3: [150], 4: [100, 130]}, absent={}, di=di, tri=tri,
                  no_di={0: [(1500, 1515), (1800, 1830), (2400, 2459)], 2: [(1500, 1801)]}, mean_len=(0, tot, n))
    return dict(chroms=chroms, alns=a, opts=[DFLT], expect=[expect])


def pe_form():
    """(f) the alignments of (c) as PE records (pr[i].hit, pr[i].nar) with interleaved reads; the oracle takes the same flat"""
    return dict(haplotypes(), pe=True)


# ---- (d) skips ---------------------------------------------------------------------------------------------------------------------
def skips():
    """(d) ten 61-base reads with a homozygous SNP in their middle on each of four sequences: m00's flagged as InDel or splice
    alignments, m01's reaching one base over the sequence's end (two of them with a trimmed high end: the whole read reaches four
    bases over it, what is left of it one), m02's with every NAR but 1, m03's ordinary.
    Ends up with: one called locus, m03's; the WIG holds m03's spans alone."""
    rng = np.random.default_rng(0x5C1)
    chroms = [rng.integers(0, 4, n).astype(np.uint8) for n in (300, 200, 300, 300)]
    alns = []
    for j, fl in enumerate([EXT_INDEL] * 3 + [EXT_SPLICE] * 3 + [EXT_INDEL | EXT_NONORPHAN, EXT_SPLICE | EXT_NONORPHAN, EXT_INDEL | (1 << 26), EXT_SPLICE | EXT_CHIMERIC]):
        alns += stack(0, chroms[0], 100, 160, ["A"], [130], flags=fl, first_minus=j)
    over = np.concatenate([chroms[1], chroms[1][:8]])  # (what lies behind the end is never looked at)
    for j in range(8):
        alns += stack(1, over, 140, 200, ["A"], [170], first_minus=j)
    for j in range(2):
        alns += stack(1, over, 143, 203, ["A"], [170], trail=3, flags=EXT_CHIMERIC, first_minus=j)
    for j, nar in enumerate((0, 2, 3, 4, 5, 6, 7, 8, 9, 10)):
        x = stack(2, chroms[2], 100, 160, ["A"], [130], first_minus=j)
        x[0][7] = nar
        alns += x
    alns += stack(3, chroms[3], 100, 160, ["A"] * 10, [130])
    expect = dict(called={0: [], 1: [], 2: [], 3: [130]}, absent={})
    return dict(chroms=chroms, alns=alns, opts=[DFLT], expect=[expect])


# ---- (e) coverage ------------------------------------------------------------------------------------------------------------------
COV_OPTS = dict(DFLT, snp_nonref_pcnt=5.0)
COV_DEEP = (255, 256, 70000)
COV_LONG = 200300
COV_SHORT = 16


def coverage():
    """(e) m00, m01, m02: 255, 256 and 70000 reads of 30 bases over loci 100..129 (coverage in one, two and four bytes).  Every
    read of m00 and m01 shows a substitution at 115, so the span is closed and written; of m02's, 7000 do: Binomial takes n > 5000
    (k becomes (int)(1000.0 / 70000 * 7000), about 100) -- a tenth, hence -1 5 for this scenario.  (With a quarter of the reads k
    would be 250, and the reference's double n-choose-k of 5000 is infinite from k = 162 on while its p^k is 0: the sum, the p-value
    and the order of its sort are no longer defined, so that input is left out.)
    m03: 200300 bases, six reads deep from locus 0 to its end, a SNP at 150000: the span from locus 0 is lost, the next one is cut
    at 100000 loci, the third is the closed tail.
    m04..m19: 140 + 3 k bases, six deep from locus 3, nine deep over the second half; the even ones with a SNP, so only they close
    the span over the second half.  Twenty WIG jobs in all.
    Ends up with: 12 called loci; m03's spans (100000, 100000, 6) and (200000, 300, 6)."""
    rng = np.random.default_rng(0xC0F)
    lens = [400, 400, 400, COV_LONG] + [140 + 3 * k for k in range(COV_SHORT)]
    chroms = [rng.integers(0, 4, n).astype(np.uint8) for n in lens]
    alns = []
    for c, n in enumerate(COV_DEEP):
        ref = chroms[c][100:130].copy()
        alt = ref.copy()
        alt[15] = other(ref[15])
        n_alt = n if n < 1000 else n // 10
        alns += [[c, 100, alt if j < n_alt else ref, bool(j & 1), 0, 0, 0, 1] for j in range(n)]  # (the reads share two arrays)
    alns += tiled(3, chroms[3], 6)
    put(alns, 3, 150000, other(chroms[3][150000]))
    called = {0: [115], 1: [115], 2: [115], 3: [150000]}
    for c in range(4, 4 + COV_SHORT):
        t = chroms[c]
        part = tiled(c, t, 6, first=3, max_len=50) + tiled(c, t, 3, first=len(t) // 2, max_len=50)
        called[c] = []
        if not c & 1:
            put(part, c, 40, other(t[40]))
            called[c] = [40]
        alns += part
    expect = dict(called=called, absent={})
    return dict(chroms=chroms, alns=alns, opts=[COV_OPTS], expect=[expect])


SCENARIOS = dict(windows=windows, thresholds=thresholds, haplotypes=haplotypes, skips=skips, coverage=coverage, pe_form=pe_form, vcf=vcf)
CASES = [("windows", 0), ("thresholds", 0), ("thresholds", 1), ("haplotypes", 0), ("skips", 0), ("coverage", 0), ("pe_form", 0), ("vcf", 0)]


@functools.lru_cache(maxsize=None)
def scenario(name):
    """the scenario with its inputs materialised: adds names, reads, rr, hits (nar = rr["nar"]), piled, and pe_reads / pe_recs"""
    s = dict(SCENARIOS[name]())
    s.setdefault("pe", False)
    s.setdefault("vcf", False)
    s["names"] = names_of(s["chroms"])
    s["reads"], s["rr"], s["hits"], s["piled"] = materialise(s["alns"])
    if s["pe"]:
        s["pe_reads"], s["pe_recs"] = as_pe(s["reads"], s["rr"], s["hits"])
    return s


def oracle_files(oracle, s, k):
    """the oracle's four texts and its count for option set k of a materialised scenario"""
    h = oracle.build(s["names"], s["chroms"])
    try:
        if s["pe"]:
            args = (h, s["pe_reads"], s["pe_recs"]["nar"].copy(), s["pe_recs"]["hit"].copy())
        else:
            args = (h, s["reads"], s["rr"]["nar"].copy(), s["hits"])
        kw = s["opts"][k]
        snp, n = oracle.snp_csv(*args, vcf=s["vcf"], **kw)
        return dict(snp=snp, n_snps=n, wig=oracle.snp_wig(*args, **kw), disnp=oracle.snp_haplotypes(args[0], 2, *args[1:], **kw),
                    trisnp=oracle.snp_haplotypes(args[0], 3, *args[1:], **kw))
    finally:
        oracle.close(h)
