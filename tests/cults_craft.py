"""Crafted cultivars and cases for CSfxArray::GenKMerCultsCnts / GenKMerCultThreadRange (tests/cults_ref.py restates them,
tests/golden/make_golden_cults.py records the reference's answers, test_cults_cpu.py and test_gpu_cults.py compare).

Five cultivars of 700 to 1900 bases that descend from one ancestor, with planted sites.  At the main geometry P = 12, S = 6:
  shared / subset      the ancestor's K-mers are in all five; point mutations leave some in a subset
  N in a prefix        cultB carries an N inside ancestral sequence
  head with N          M1 + "AN" (cultC) sorts in front of M1 + "CG.." (cultA, cultB): the run's first element is no head
  member with N        M1 + "TN" (cultD) sorts last in that run and is skipped
  split run            cultE, the last entry, ends with M2 + "AAA": fewer than S bases follow, the element is too short, and it sorts
                       between M2 + "AAAC.." (cultA) and M2 + "TTTG.." (cultB), so that K-mer is located twice
  palindrome           PAL is its own reverse complement (cultA, cultC): its loci count again as antisense
  antisense only       M3 is in cultA and cultB; cultD has only its reverse complement
  antisense with N     cultE has the reverse complement of M3 followed by "AN": rejected when S > 0, counted when S = 0
  repeat               a 20-base unit 30 times over in cultB
  homopolymer          150 A in cultC (one run of more than 64 elements), 100 T in cultD (an antisense range of more than 64)
"""
import numpy as np

N_ = 4
P, S = 12, 6
NAMES = ["cultA", "cultB", "cultC", "cultD", "cultE"]


def _codes(s):
    return np.array(["ACGTN".index(c) for c in s], dtype=np.uint8)


def _rc(a):
    a = np.asarray(a, dtype=np.uint8)[::-1].copy()
    m = a <= 3
    a[m] = 3 - a[m]
    return a


M1 = _codes("GATTACAGGCTA")
M2 = _codes("CCATGGTTCAGA")
M3 = _codes("TGGACCTAGTCA")
PAL = _codes("ACGTTGCAACGT")
UNIT = _codes("GTCAGGATCCTAGCATTGCA")


def targets():
    rng = np.random.default_rng(20260)
    anc = rng.integers(0, 4, 600).astype(np.uint8)

    def filler(n):
        return rng.integers(0, 4, n).astype(np.uint8)

    def mutated(k):
        a = anc.copy()
        for p in rng.choice(len(a), k, replace=False):
            a[p] = (a[p] + 1 + rng.integers(0, 3)) % 4
        return a

    b_anc = mutated(6)
    b_anc[300] = N_
    a = np.concatenate([anc, M1, _codes("CGTAGC"), filler(20), M2, _codes("AAACGT"), filler(20), PAL, filler(25), M3, _codes("GATCGA"), filler(30)])
    b = np.concatenate([b_anc, M1, _codes("CGATCA"), filler(15), M2, _codes("TTTGCA"), filler(15), M3, _codes("CCGTAT"), filler(10), np.tile(UNIT, 30),
                        filler(40), anc[100:500]])
    c = np.concatenate([mutated(9), filler(10), M1, _codes("ANGTCA"), filler(12), PAL, filler(10), np.zeros(150, np.uint8), filler(30), anc[:300]])
    d = np.concatenate([mutated(12), M1, _codes("TNACGT"), filler(10), _rc(np.concatenate([M3, _codes("GATCGA")])), filler(10), np.full(100, 3, np.uint8),
                        filler(20)])
    e = np.concatenate([mutated(4)[:560], filler(30), _rc(M3), _codes("ANCCGT"), filler(20), anc[200:260], M2, _codes("AAA")])
    return NAMES, [a, b, c, d, e]


def cases():
    """(name, kwargs of gen_kmer_cults_cnts, range): range is (start, end) or a word that resolve() turns into one"""
    def kw(sense_only=False, plen=P, slen=S, min_cult=0, max_homo=0):
        return dict(sense_only=sense_only, plen=plen, slen=slen, min_cult=min_cult, max_homo=max_homo)

    out = [("all_cultivars", kw(), (0, 0)), ("min3", kw(min_cult=3), (0, 0)), ("min1", kw(min_cult=1), (0, 0)), ("min5_is_all", kw(min_cult=5), (0, 0)),
           ("min2_end_n1", kw(min_cult=2), "end_n1"), ("sense_only_min1", kw(True, min_cult=1), (0, 0)), ("sense_only_all", kw(True), (0, 0)),
           ("no_suffix_min1", kw(slen=0, min_cult=1), (0, 0)), ("no_suffix_homo_ignored", kw(slen=0, min_cult=4, max_homo=2), (0, 0)),
           ("p5_min1", kw(plen=5, slen=0, min_cult=1), (0, 0)), ("p5_s5", kw(plen=5, slen=5, min_cult=2), (0, 0)),
           ("p200_s100", kw(plen=200, slen=100, min_cult=1), (0, 0)), ("p20_s4_min2", kw(plen=20, slen=4, min_cult=2), (0, 0)),
           ("mid_run", kw(min_cult=1), "mid_run"), ("mid_run_sense", kw(True, min_cult=1), "mid_run"), ("start_eq_n", kw(min_cult=1), "start_n"),
           ("one_element", kw(min_cult=1), "one_element"), ("tail", kw(min_cult=1), "tail")]
    for nt in (1, 2, 3, 4):
        for t in range(1, nt + 1):
            out.append(("threads_%d_%d" % (nt, t), kw(min_cult=1), ("thread", nt, t)))
    errs = [dict(plen=4), dict(slen=-1), dict(plen=201, slen=0), dict(plen=100, slen=201), dict(min_cult=-1), dict(plen=200, slen=101), dict(min_cult=6)]
    out += [("err_%d" % i, kw(**e), (0, 0)) for i, e in enumerate(errs)]
    out += [("err_start_neg", kw(), (-1, 0)), ("err_end_neg", kw(), (0, -1)), ("err_start_past", kw(), "start_past")]
    out.append(("homozygotic_unsupported", kw(max_homo=1), (0, 0)))
    return out


def longest_run(index, plen=P):
    """(first, last) suffix indices of the longest run of suffixes that share plen ACGT bases"""
    seq, sa, _ = index
    best, s = (0, 0), 0
    key = lambda i: bytes(seq[sa[i]:sa[i] + plen])
    for i in range(1, len(sa) + 1):
        if i == len(sa) or key(i) != key(s):
            if i - 1 - s > best[1] - best[0] and len(key(s)) == plen and max(key(s)) <= 3:
                best = (s, i - 1)
            s = i
    return best


def resolve(rng, index, thread_range):
    """the (start, end) of a case, or None where GenKMerCultThreadRange leaves the thread nothing (rc < 1)"""
    n = len(index[0])
    if isinstance(rng, tuple) and rng[0] == "thread":
        start = 0
        for t in range(1, rng[2] + 1):
            rc, end = thread_range(index, P, t, rng[1], start)
            if rc < 1:
                return None
            if t == rng[2]:
                return start, end
            start = end + 1
    if isinstance(rng, tuple):
        return rng
    lo, hi = longest_run(index)
    return {"end_n1": (0, n - 1), "mid_run": (lo + (hi - lo) // 3, hi - (hi - lo) // 4), "start_n": (n, 0), "start_past": (n + 1, 0),
            "one_element": (lo + 2, lo + 2), "tail": (n - 40, n + 5)}[rng]


BIG_NAMES = ["big%d" % i for i in range(6)]
BIG_THREADS = (2, 3, 4)


def big_targets():
    """six cultivars of 17 000 bases, 3 % apart from one ancestor: 102 006 suffix array elements, enough for GenKMerCultThreadRange to
    give each of four threads a range of its own; nearly every 12-mer is a run of several elements, so the putative boundaries fall
    inside runs and the search for the next K-mer has to move them"""
    rng = np.random.default_rng(20263)
    anc = rng.integers(0, 4, 17000).astype(np.uint8)
    out = []
    for _ in BIG_NAMES:
        t = anc.copy()
        pos = rng.choice(len(t), size=len(t) * 3 // 100, replace=False)
        t[pos] = (t[pos] + rng.integers(1, 4, len(pos))) % 4
        out.append(t)
    return BIG_NAMES, out


def thread_ranges(index, thread_range, nt, klen=P):
    """[(t, start, rc, end)] as CMarkerKMers::LocKMers partitions (MarkerKMers.cpp:449-458): the loop ends at the first rc < 1"""
    rows, start = [], 0
    for t in range(1, nt + 1):
        rc, end = thread_range(index, klen, t, nt, start)
        rows.append((t, start, rc, end))
        if rc < 1:
            break
        start = end + 1
    return rows
