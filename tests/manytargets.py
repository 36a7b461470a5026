"""Seeded genomes of many small targets and the reads that go with them (numpy, CPU): the inputs of the tests that take the
alignment, pairing and formatting code past K4_LDS_ENTRIES (128) targets, where MapChunkHit2Entry searches the entry table in
global memory (test_manytargets_cpu.py, test_gpu_manytargets.py, tests/golden/make_golden_manytargets.py).

genome(n) is the first n targets of ONE sequence of targets (target i is drawn from its own generator), so the 128-, 129- and
300-target indexes share their leading targets.  Target indices are 0-based here; the chrom_id of a hit is index + 1, so the
targets of index >= 128 are the ones with id > 128.  About 150 kbp at 300 targets:

  3, 4, 5 / 131, 132, 133        targets shorter than any read: 1, 7 and 40 bases
  6..13 / 134..141               for each read length L of RAW_LENS a target of exactly L bases, then one of L - 1 (the second must be
                                 rejected by the end-of-entry test  left + len - 1 > e_end)
  (125, 130) and (150, 220)      two pairs of byte-identical targets (the first straddles index 128): a read drawn from them has two
                                 instances that differ only in chrom_id
  16, 60 / 144, 230              2 500 bases (reads over 512 bp); 60 and 230 carry an N run in the middle
  17 / 145                       an N run touching the target's last base
  30, 70, 100, 120 / 142, 155,   at least 800 bases, with one and the same 200 bases at 250..449: 12 exact copies, more than the 10 hit slots
  170, 190, 205, 225, 245, 265   of the paired-end flow, so a mate inside them is multi-aligned and can only be placed by the mate rescue
  0, 1, 126..129, 298, 299       ordinary, at least 450 bases (every RAW_LENS read fits at both ends)
  the rest                       ordinary, 200 to 1 500 bases, short ones far more frequent
"""
import hashlib

import numpy as np

import synth

SEED = 0x4D543330  # "MT30"
RAW_LENS = (100, 150, 250, 400)
# AlignReads arguments per read length of RAW_LENS: (TotMM, CoreLen, CoreDelta, MaxNumCoreSlides)
RAW_ARGS = {100: (2, 33, 33, 8), 150: (3, 37, 37, 12), 250: (5, 41, 41, 21), 400: (6, 57, 57, 30)}
NPZ_CASES = ("mt300_se_s2", "mt300_s3_150_mh10")  # tests/golden/align_<case>.npz: what the reference's AlignReads returned
TINY = {3: 1, 4: 7, 5: 40, 131: 1, 132: 7, 133: 40}
EXACT = {}  # index -> (read length, target length)
for _k, _L in enumerate(RAW_LENS):
    for _base in (6, 134):
        EXACT[_base + 2 * _k] = (_L, _L)
        EXACT[_base + 2 * _k + 1] = (_L, _L - 1)
DUPLICATES = ((125, 130), (150, 220))
LONG = (16, 60, 144, 230)
N_MIDDLE = (60, 230)
N_TAIL = (17, 145)
N_TAIL_LEN = 25
REPEAT_TARGETS = (30, 70, 100, 120, 142, 155, 170, 190, 205, 225, 245, 265)
REPEAT_AT, REPEAT_LEN = 250, 200
END_TARGETS = (0, 1, 126, 127, 128, 129)  # and n - 2, n - 1


def _target(i):
    rng = np.random.default_rng([SEED, i])
    if i in TINY:
        ln = TINY[i]
    elif i in EXACT:
        ln = EXACT[i][1]
    elif i in LONG:
        ln = 2500
    elif any(i in p for p in DUPLICATES):
        ln = 600
    elif i in N_TAIL:
        ln = 800
    else:
        ln = 200 + int(1300 * rng.random() ** 3.5)
        if i in END_TARGETS or i in (298, 299):
            ln = max(ln, 450 + i % 7)
        if i in REPEAT_TARGETS:
            ln = max(ln, 800 + i % 11)
    t = rng.integers(0, 4, size=ln, dtype=np.uint8)
    if i in REPEAT_TARGETS:
        t[REPEAT_AT:REPEAT_AT + REPEAT_LEN] = np.random.default_rng([SEED, 1 << 20]).integers(0, 4, size=REPEAT_LEN, dtype=np.uint8)
    if i in N_MIDDLE:
        t[1200:1230] = 4
    if i in N_TAIL:
        t[ln - N_TAIL_LEN:] = 4
    return t


def genome(n):
    """(names, targets) of the n-target genome"""
    chroms = [_target(i) for i in range(n)]
    for a, b in DUPLICATES:
        if b < n:
            chroms[b] = chroms[a].copy()
    return ["t%05d" % (i + 1) for i in range(n)], chroms


def small_genome(n, seed=SEED + 1):
    """n targets of 120 to 400 bases (the 12 000-target index: a binary search 14 levels deep)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(120, 401, n)
    return ["s%05d" % (i + 1) for i in range(n)], [rng.integers(0, 4, int(ln)).astype(np.uint8) for ln in lens]


def end_targets(n):
    return sorted(set(t for t in END_TARGETS + (n - 2, n - 1) if 0 <= t < n))


def end_reads(chroms, read_len):
    """Reads that start at locus 0 and reads that end at the last base of the END_TARGETS, on both strands, without substitutions.
    Returns (reads, truth[chrom(1-based), start, strand, 0]) as synth.make_reads does."""
    reads, truth = [], []
    for t in end_targets(len(chroms)):
        c = chroms[t]
        if len(c) < read_len:
            continue
        for start in (0, len(c) - read_len):
            for strand in (0, 1):
                rd = c[start:start + read_len].copy()
                reads.append(synth.revcomp(rd) if strand else rd)
                truth.append((t + 1, start, strand, 0))
    return reads, np.array(truth, dtype=np.int64).reshape(-1, 4)


def beyond_reads(chroms, read_len, seed=SEED + 2):
    """Reads that would need one base beyond a target's end (the last read_len - 1 bases, then a foreign base) or one before its
    start (a foreign base, then the first read_len - 1 bases), on both strands: over the END_TARGETS and, whole, over the targets
    of read_len - 1 bases.  Returns (reads, rows[chrom(1-based), the locus such a placement would have to report])."""
    rng = np.random.default_rng(seed)
    reads, rows = [], []
    short = [i for i, (L, ln) in EXACT.items() if L == read_len and ln == read_len - 1 and i < len(chroms)]
    for t in end_targets(len(chroms)) + short:
        c = chroms[t]
        if len(c) < read_len - 1:
            continue
        x = rng.integers(0, 4, size=2, dtype=np.uint8)
        for rd, loci in ((np.concatenate([c[len(c) - read_len + 1:], x[:1]]), len(c) - read_len + 1),
                         (np.concatenate([x[1:], c[:read_len - 1]]), 0)):
            for strand in (0, 1):
                reads.append(synth.revcomp(rd) if strand else rd.copy())
                rows.append((t + 1, loci))
    return reads, np.array(rows, dtype=np.int64).reshape(-1, 2)


def exact_target_reads(chroms, read_len):
    """the whole target of exactly read_len bases, on both strands, each side of 128: (reads, truth) as end_reads"""
    reads, truth = [], []
    for i, (L, ln) in sorted(EXACT.items()):
        if L == read_len and ln == read_len and i < len(chroms):
            for strand in (0, 1):
                reads.append(synth.revcomp(chroms[i]) if strand else chroms[i].copy())
                truth.append((i + 1, 0, strand, 0))
    return reads, np.array(truth, dtype=np.int64).reshape(-1, 4)


def duplicate_reads(chroms, n_reads, read_len, seed=SEED + 3, sub_lambda=0.5):
    """reads drawn from the duplicated targets: (reads, pair[n]: index into DUPLICATES)"""
    rng = np.random.default_rng(seed)
    pairs = [k for k, (a, b) in enumerate(DUPLICATES) if b < len(chroms)]
    reads, which = [], []
    for _ in range(n_reads if pairs else 0):
        k = pairs[int(rng.integers(0, len(pairs)))]
        c = chroms[DUPLICATES[k][int(rng.integers(0, 2))]]
        start = int(rng.integers(0, len(c) - read_len + 1))
        rd = c[start:start + read_len].copy()
        for p in rng.choice(read_len, size=int(min(rng.poisson(sub_lambda), 2)), replace=False):
            rd[p] = (rd[p] + int(rng.integers(1, 4))) % 4
        reads.append(synth.revcomp(rd) if rng.random() < 0.5 else rd)
        which.append(k)
    return reads, np.array(which, dtype=np.int64)


def raw_batch(chroms, n_reads, read_len, seed, crafted=True):
    """a uniform-length batch for AlignReads: make_reads over all targets (substitutions, N, end-hugging and foreign reads), then
    the crafted reads (crafted=False, for a genome other than genome(n): the end reads only).  Returns (reads, dict of the index
    ranges of the crafted groups and their truth)."""
    reads, truth = synth.make_reads(chroms, n_reads, read_len, seed=seed, sub_lambda=max(1.0, read_len / 100.0), n_prob=0.03,
                                    edge_frac=0.1, random_frac=0.03)
    groups = {"random": (0, len(reads), truth)}
    more = [("ends", end_reads(chroms, read_len))]
    if crafted:
        more += [("exact", exact_target_reads(chroms, read_len)), ("beyond", beyond_reads(chroms, read_len)),
                 ("dup", duplicate_reads(chroms, 200, read_len, seed=seed + 1))]
    for name, (r, t) in more:
        groups[name] = (len(reads), len(reads) + len(r), t)
        reads = reads + r
    return reads, groups


def mixed_batch(chroms, seed, scale=1.0, crafted=True):
    """36 to 2 000 bp reads in one batch (no longer than the longest target), reads with N included: the step kernels' classes, reads
    the general kernel answers (N, over 512 bp) and reads too short or too long for most targets"""
    reads = []
    longest = max(len(c) for c in chroms)
    for rl, nr in ((36, 300), (50, 400), (75, 400), (100, 900), (129, 300), (151, 500), (250, 400), (400, 300), (513, 250), (700, 200),
                   (1200, 120), (2000, 80)):
        if rl > longest:
            continue
        r, _ = synth.make_reads(chroms, max(8, int(nr * scale)), rl, seed=seed + rl, sub_lambda=max(1.0, rl / 120.0), n_prob=0.15,
                                edge_frac=0.1, random_frac=0.03)
        reads += r
    for rl in (100, 400):
        reads += end_reads(chroms, rl)[0] + (beyond_reads(chroms, rl)[0] if crafted else [])
    return reads + (duplicate_reads(chroms, 150, 120, seed=seed + 7)[0] if crafted else [])


def _mutate(rd, rng, ns):
    for p in rng.choice(len(rd), size=ns, replace=False):
        if rd[p] <= 3:
            rd[p] = (rd[p] + int(rng.integers(1, 4))) % 4
    return rd


def pe_batch(chroms, n_pairs, read_len=100, seed=SEED + 4, frag_min=220, frag_max=420, crafted=True):
    """Paired reads: synth.make_pe_reads over all targets long enough, then `rescue` pairs on REPEAT_TARGETS of index >= 128 with one
    end inside the 12-copy repeat (multi-aligned: it can only be placed by the mate rescue, next to its unique mate), then `cross` pairs
    whose ends lie on different targets (crafted=False, for a genome other than genome(n): no rescue pairs).  Returns (pe1, pe2, kind[n]: 0 ordinary / 1 rescue / 2 cross, target index of PE1)."""
    pe1, pe2, truth = synth.make_pe_reads(chroms, n_pairs, read_len, seed=seed, frag_min=frag_min, frag_max=frag_max, sub_lambda=1.2,
                                          n_prob=0.02, random_mate_frac=0.03)
    kind, targ = [0] * n_pairs, list(truth[:, 0] - 1)
    rng = np.random.default_rng(seed + 1)
    high = [i for i in REPEAT_TARGETS if 128 <= i < len(chroms)] if crafted else []
    long_enough = [i for i in range(len(chroms)) if len(chroms[i]) >= read_len and not (chroms[i] > 3).any()]
    for _ in range(n_pairs // 5 if high else 0):  # one end inside the repeat, the other in the unique sequence behind it
        t = high[int(rng.integers(0, len(high)))]
        start = int(rng.integers(REPEAT_AT, REPEAT_AT + REPEAT_LEN - read_len + 1))
        flen = int(rng.integers(max(frag_min, REPEAT_AT + REPEAT_LEN + read_len - start), frag_max + 1))
        frag = chroms[t][start:start + flen]
        if rng.random() < 0.5:
            frag = synth.revcomp(frag)
        pe1.append(_mutate(frag[:read_len].copy(), rng, int(rng.integers(0, 3))))
        pe2.append(_mutate(synth.revcomp(frag[flen - read_len:]), rng, int(rng.integers(0, 3))))
        kind.append(1)
        targ.append(t)
    for _ in range(n_pairs // 10 if len(long_enough) > 1 else 0):
        a, b = (long_enough[int(q)] for q in rng.choice(len(long_enough), size=2, replace=False))
        sa, sb = (int(rng.integers(0, len(chroms[t]) - read_len + 1)) for t in (a, b))
        ra, rb = chroms[a][sa:sa + read_len].copy(), synth.revcomp(chroms[b][sb:sb + read_len])
        if rng.random() < 0.5:
            ra, rb = synth.revcomp(ra), synth.revcomp(rb)
        pe1.append(_mutate(ra, rng, int(rng.integers(0, 2))))
        pe2.append(_mutate(rb, rng, int(rng.integers(0, 2))))
        kind.append(2)
        targ.append(a)
    return pe1, pe2, np.array(kind), np.array(targ)


def chimeric_reads(chroms, n_reads, read_len, seed=SEED + 5):
    """synth.make_ext_reads('chimeric') drawn from the targets of index >= 128 only; the targets keep their ids because the reads
    are cut from the sequences, not placed by index"""
    return synth.make_ext_reads(chroms[128:], n_reads, read_len, "chimeric", seed=seed, max_subs=2)


def repeat_reads(chroms, n_multi, n_flank, read_len=100, seed=SEED + 6, favoured=(170,)):
    """for AssignMultiMatches: n_multi reads from inside the 12-copy repeat (every copy is an instance), and n_flank uniquely aligned
    reads that overlap the repeat's edges on each of the `favoured` targets, which give those copies the neighbours the others lack"""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n_multi):
        c = chroms[REPEAT_TARGETS[int(rng.integers(0, len(REPEAT_TARGETS)))]]
        start = int(rng.integers(REPEAT_AT, REPEAT_AT + REPEAT_LEN - read_len + 1))
        rd = _mutate(c[start:start + read_len].copy(), rng, int(rng.integers(0, 2)))
        reads.append(synth.revcomp(rd) if rng.random() < 0.5 else rd)
    for t in favoured:
        for _ in range(n_flank):
            left = rng.random() < 0.5
            start = int(rng.integers(REPEAT_AT - 70, REPEAT_AT - 30)) if left else int(rng.integers(REPEAT_AT + REPEAT_LEN - read_len + 30,
                                                                                                   REPEAT_AT + REPEAT_LEN - read_len + 70))
            rd = chroms[t][start:start + read_len].copy()
            reads.append(synth.revcomp(rd) if rng.random() < 0.5 else rd)
    return reads


def sa_ties_by_offset(seq, sa):
    """A 4-byte suffix array with every run of suffixes that compare equal (identical through their first EOS, symbol 7: the
    reference's comparison stops there and its quicksort leaves such suffixes in any order) put in offset order: two arrays over
    the same sequence are the same up to that freedom iff this form of them is equal."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    sa = np.array(sa, dtype=np.int64)
    eos = np.flatnonzero(seq == 7)
    end = eos[np.searchsorted(eos, sa)]  # the EOS that closes each suffix (the concatenation ends with one)
    raw = seq.tobytes()
    same = np.zeros(len(sa), dtype=bool)  # same[i]: suffix i compares equal to suffix i - 1
    cand = np.flatnonzero((end - sa)[1:] == (end - sa)[:-1]) + 1
    for i in cand:
        same[i] = raw[sa[i]:end[i]] == raw[sa[i - 1]:end[i - 1]]
    group = np.cumsum(~same)
    return sa[np.lexsort((sa, group))].astype("<u4")


def sfx_parts(raw):
    """SHA-256 of the parts of an .sfx with 4-byte suffix elements (layout: test_oracle_golden.py::
    test_sfx_reader_and_writer_roundtrip), so that two files can be compared without keeping either: fixed header fields, dataset
    name, free header text, block header and sequence, suffix array, entries -- and the suffix array in its sa_ties_by_offset form"""
    n = int.from_bytes(raw[1224 + 8:1224 + 16], "little")
    s0 = 1224 + 20
    cuts = {"fields": (0, 52), "dataset": (52, 133), "text": (133, 1224), "block": (1224, s0 + n), "sa": (s0 + n, s0 + 5 * n),
            "entries": (s0 + 5 * n, len(raw))}
    parts = {k: hashlib.sha256(raw[a:b]).hexdigest() for k, (a, b) in cuts.items()}
    parts["sa_ties_by_offset"] = hashlib.sha256(sa_ties_by_offset(np.frombuffer(raw[s0:s0 + n], dtype=np.uint8),
                                                                  np.frombuffer(raw[s0 + n:s0 + 5 * n], dtype="<u4")).tobytes()).hexdigest()
    return parts


def rescue_calls(chroms, targets, rng, per_target=8, read_len=100, lo=150, hi=500, max_mm=2):
    """AlignPairedRead calls (the mate rescue next to an anchor) on made-up anchors, per_target on each of `targets` (every one at
    least lo + 20 bases): a fragment of lo + 20 to hi bases, three in ten flush with an end of the target, the anchor its left end
    and the mate 3' of it or the other way round, the mate with 0 to 3 substitutions (3 are more than max_mm = 2 allows) on either
    strand.  Returns [(target index, b3prime_extend, antisense, anchor start, anchor end, lo, hi, max_mm, mate)]."""
    calls = []
    for t in targets:
        c = chroms[t]
        for _ in range(per_target):
            flen = int(rng.integers(lo + 20, min(hi, len(c)) + 1))
            start = int(rng.integers(0, len(c) - flen + 1)) if rng.random() < 0.7 else int(rng.choice([0, len(c) - flen]))
            b3 = int(rng.integers(0, 2))
            a_start = start if b3 else start + flen - read_len
            m_start = start + flen - read_len if b3 else start
            mate = c[m_start:m_start + read_len].copy()
            for p in rng.choice(read_len, size=int(rng.integers(0, 4)), replace=False):
                mate[p] = (mate[p] + int(rng.integers(1, 4))) % 4
            anti = int(rng.integers(0, 2))
            if anti:
                mate = synth.revcomp(mate)
            calls.append((int(t), b3, anti, a_start, a_start + read_len - 1, lo, hi, max_mm, np.ascontiguousarray(mate, dtype=np.uint8)))
    return calls


RESCUE_CHIMERIC = (50, 33, 33)  # MinChimericLen, CoreLen, CoreDelta of the chimeric calls (100 bp mates, as `-c50 -s2` derives them)


def chimeric_rescue_calls(chroms, rng, per_target=6):
    """rescue_calls for AlignPairedRead's chimeric mode on the targets of 1 300 bases and more, with insert windows up to 1 500 loci:
    windows of 1 000 loci and more are seeded with exact cores from the suffix array and every seed is mapped to its target, smaller
    ones are scanned; a third of the mates carry 20 to 35 foreign bases at their start, so only a trimmed placement exists"""
    calls = rescue_calls(chroms, [t for t in range(len(chroms)) if len(chroms[t]) >= 1300], rng, per_target=per_target, hi=1500)
    for k in range(0, len(calls), 3):
        flank = int(rng.integers(20, 36))
        calls[k][-1][:flank] = rng.integers(0, 4, flank)
    return calls
