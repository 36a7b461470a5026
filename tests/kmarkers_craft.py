"""A crafted index and the cases for `ngskit4b kmarkers` (CLocKMers::LocateSpeciesUniqueKMers) and the CSfxArray calls under it
(tests/kmarkers_ref.py restates them, tests/golden/make_golden_kmarkers.py records the reference, test_kmarkers_cpu.py and
test_gpu_kmarkers.py compare).

Six entries of 1000 to 2000 bases; entries 2 ("Tgt_b") and 4 ("tgt_A") are the target cultivar.  The front end sorts the names
without case, so tgt_A is processed first although it is the later entry, and although 'T' < 't'.  Every entry is random
sequence of its own with planted sites between; sites() tells where each stands and what it was made for.
  acc        a 50-mer only in tgt_A
  dup        a 50-mer in tgt_A, again later in tgt_A, and in Tgt_b
  rcdup      a 50-mer in tgt_A whose reverse complement is in Tgt_b (duplicate through the second flag)
  pal        a 50-base palindrome in tgt_A: every centred even-length window is its own reverse complement
  rcf1/rcf2  a 50-mer in tgt_A whose reverse complement is in one / in two other entries (the walk skips the first antisense hit)
  ff / fh    a 50-mer in o1 and tgt_A, o1's copy sorting first / last
  homo       150 A in tgt_A: runs of more than 64 elements
  nruns      ACGT runs of K - 1, K, K + 1 bases between Ns for K = 20, 25, 50 in Tgt_b; tgt_A ends with N + 20 bases, Tgt_b with N + 51
  ham*       (K = 50, MinHamming 3: cores of 16 at 0, 16, 32) a foreign hit of core 16 that can be extended; the same within 5 bases
             of an entry's start; within 26 of an entry's end; a foreign copy of bases 25..49 (at MinHamming 2 the only core is 0);
             a foreign hit of the reverse complement's core 0
  px0/1/3    (K = 50, prefix 20) the first 20 bases shared with no other entry, with o1, with o1 and o2 and -- as the reverse
             complement of the last 20 -- o3
  runs       (K = 20) in Tgt_b a stretch whose 20-mers at chosen starts stand, each alone between Ns, in tgt_A as well: accepted runs
             of 1, 2 and 5 with duplicates between, and one more accepted K-mer behind
"""
import numpy as np

N_ = 4
NAMES = ["o1", "Tgt_b", "o2", "tgt_A", "o3", "o4"]
CULTIVAR = "tgt"
TARGET_NAMES = ["Tgt_b", "tgt_A"]  # as given on the command line; processed as tgt_A, Tgt_b
RUN_PATTERN = "DADAADAAAAADAD"   # the stretch's starts: Accepted / Duplicate


def _rc(a):
    a = np.asarray(a, dtype=np.uint8)[::-1].copy()
    m = a <= 3
    a[m] = 3 - a[m]
    return a


def build():
    """(names, sequences, sites): sites[name] = (entry id, locus) of the site's first base"""
    rng = np.random.default_rng(20271)

    def rnd(n):
        return rng.integers(0, 4, n).astype(np.uint8)

    n1 = np.array([N_], dtype=np.uint8)
    parts = {n: [] for n in NAMES}
    sites = {}

    def put(name, *chunks, site=None):
        if site:
            sites[site] = (NAMES.index(name) + 1, sum(len(c) for c in parts[name]))
        parts[name].extend(np.asarray(c, dtype=np.uint8) for c in chunks)

    m = {k: rnd(50) for k in ("acc", "dup", "rcdup", "rcf1", "rcf2", "ff", "fh", "ham1", "ham_start", "ham_end", "ham_last", "ham_rc", "px1", "px3")}
    half = rnd(25)
    pal = np.concatenate([half, _rc(half)])
    a_ = np.array([0], dtype=np.uint8)
    t_ = np.array([3], dtype=np.uint8)
    stretch = rnd(len(RUN_PATTERN) + 19)

    # o4 begins with the start-flank site, o1 ends with the end-flank site (below)
    put("o4", rnd(5), m["ham_start"][16:32], rnd(60))
    for name in NAMES:
        put(name, rnd(120))
    # tgt_A (processed first)
    put("tgt_A", m["acc"], rnd(40), site="acc")
    put("tgt_A", m["dup"], rnd(40), site="dup")
    put("tgt_A", m["rcdup"], rnd(40), site="rcdup")
    put("tgt_A", n1, pal, n1, rnd(40), site="pal_n")
    put("tgt_A", m["rcf1"], rnd(30), site="rcf1")
    put("tgt_A", m["rcf2"], rnd(30), site="rcf2")
    put("tgt_A", m["ff"], t_, rnd(30), site="ff")
    put("tgt_A", m["fh"], a_, rnd(30), site="fh")
    put("tgt_A", np.array([1], np.uint8), np.zeros(150, np.uint8), np.array([2], np.uint8), rnd(30), site="homo_c")
    for k in ("ham1", "ham_start", "ham_end", "ham_last", "ham_rc", "px1", "px3"):
        put("tgt_A", m[k], rnd(30), site=k)
    put("tgt_A", m["dup"], rnd(30), site="dup_again")
    for i, c in enumerate(RUN_PATTERN):
        if c == "D":
            put("tgt_A", n1, stretch[i:i + 20], site="runs_plant_%d" % i)
    put("tgt_A", n1, rnd(60), n1, rnd(20), site="tail_n")
    # Tgt_b
    put("Tgt_b", m["dup"], rnd(40), site="dup_b")
    put("Tgt_b", _rc(m["rcdup"]), rnd(40), site="rcdup_b")
    for k in (20, 25, 50):
        put("Tgt_b", n1, rnd(k - 1), n1, rnd(k), n1, rnd(k + 1), n1, rnd(30), site="nruns_%d" % k)
    put("Tgt_b", rnd(20), site="runs_lead")
    put("Tgt_b", stretch, rnd(60), site="runs")
    put("Tgt_b", n1, rnd(51), site="tail_n")
    # the others
    put("o2", _rc(m["rcf1"]), rnd(50))
    put("o2", _rc(m["rcf2"]), rnd(50))
    put("o3", _rc(m["rcf2"]), rnd(50))
    put("o1", m["ff"], a_, rnd(50))
    put("o1", m["fh"], t_, rnd(50))
    put("o3", rnd(30), m["ham1"][16:32], rnd(60))
    put("o2", rnd(40), m["ham_last"][25:50], rnd(60))
    put("o3", rnd(40), _rc(m["ham_rc"])[0:16], rnd(60))
    put("o1", rnd(30), m["px1"][0:20], rnd(60))
    put("o1", rnd(30), m["px3"][0:20], rnd(60))
    put("o2", rnd(30), m["px3"][0:20], rnd(60))
    put("o3", rnd(30), _rc(m["px3"][30:50]), rnd(60))
    for name in ("o1", "o2", "o3", "o4"):
        put(name, rnd(400))
    put("o1", rnd(20), m["ham_end"][16:32], rnd(10))
    seqs = [np.concatenate(parts[n]) for n in NAMES]
    return NAMES, seqs, sites


def target_ids():
    """the front end's processing order: qsort by stricmp of the names (LocKMers.cpp:587, :1451-1455)"""
    return [NAMES.index(n) + 1 for n in sorted(TARGET_NAMES, key=lambda s: s.lower())]


def scan_cases():
    """(name, kwargs of species_kmers): K = 20, 25, 50; MinHamming 1, 2, 3, 5 (at K = 20 with 5 the core is clamped to 8); all modes"""
    out = []
    for k in (20, 25, 50):
        for mh in (1, 2, 3, 5):
            out.append(("k%d_h%d_m0" % (k, mh), dict(kmer_len=k, min_hamming=mh, mode=0)))
        out.append(("k%d_h1_m1" % k, dict(kmer_len=k, min_hamming=1, mode=1)))
        out.append(("k%d_h2_m1" % k, dict(kmer_len=k, min_hamming=2, mode=1)))
        for s in (0, 1, 3):
            out.append(("k%d_h1_m2_s%d" % (k, s), dict(kmer_len=k, min_hamming=1, mode=2, prefix_len=10 if k == 20 else 20 if k == 50 else 12, min_with_prefix=s)))
    out.append(("k50_h2_m2_s3", dict(kmer_len=50, min_hamming=2, mode=2, prefix_len=20, min_with_prefix=3)))
    out.append(("k100_h5_m0", dict(kmer_len=100, min_hamming=5, mode=0)))
    return out


def error_cases():
    """(name, target ids or None for the crafted ones, kwargs): each gives K4_ERR_PARAMS"""
    t = None
    return [("k19", t, dict(kmer_len=19)), ("k101", t, dict(kmer_len=101)), ("h0", t, dict(kmer_len=20, min_hamming=0)),
            ("h6", t, dict(kmer_len=20, min_hamming=6)), ("p9", t, dict(kmer_len=20, mode=2, prefix_len=9)),
            ("p11_k20", t, dict(kmer_len=20, mode=2, prefix_len=11)), ("p41_k50", t, dict(kmer_len=50, mode=2, prefix_len=41)),
            ("unknown_id", [4, 7], dict(kmer_len=20)), ("id_zero", [0, 4], dict(kmer_len=20)), ("repeated_id", [4, 2, 4], dict(kmer_len=20)),
            ("all_entries", [1, 2, 3, 4, 5, 6], dict(kmer_len=20)), ("too_many", list(range(1, 52)), dict(kmer_len=20))]


def file_cases():
    """(file stem, front-end options): mode, K, -p, -s, -K as given to `ngskit4b kmarkers`; kmarkers_fasta takes the same"""
    out = []
    for k in (20, 25, 50):
        out.append(("kmarkers_k%d_m0" % k, dict(kmer_len=k, mode=0)))
        out.append(("kmarkers_k%d_m1" % k, dict(kmer_len=k, mode=1)))
    out.append(("kmarkers_k50_m0_K3", dict(kmer_len=50, mode=0, min_hamming=3)))
    for s in (0, 1, 3):
        out.append(("kmarkers_k50_m2_p20_s%d_K3" % s, dict(kmer_len=50, mode=2, prefix_len=20, min_shared=s, min_hamming=3)))
    out.append(("kmarkers_k50_m2_p20_s2_K1", dict(kmer_len=50, mode=2, prefix_len=20, min_shared=2, min_hamming=1)))
    out.append(("kmarkers_k50_m2_p20_s5_K2", dict(kmer_len=50, mode=2, prefix_len=20, min_shared=5, min_hamming=2)))
    out.append(("kmarkers_k20_m2_s1", dict(kmer_len=20, mode=2, min_shared=1)))
    out.append(("kmarkers_k25_m2_p12_s3_K4", dict(kmer_len=25, mode=2, prefix_len=12, min_shared=3, min_hamming=4)))
    return out


def probes(seqs, n=300):
    """probes for IterateExacts / MatchesOtherChroms: windows of the entries of 8 to 60 bases (some across an N or an entry's end),
    mutated copies and random sequence; [(codes, ids, MaxTotMM)]"""
    rng = np.random.default_rng(20272)
    out = []
    for i in range(n):
        e = int(rng.integers(0, len(seqs)))
        ln = int(rng.choice([8, 10, 12, 16, 20, 25, 33, 50, 60]))
        p = int(rng.integers(0, len(seqs[e]) - ln + 1))
        s = seqs[e][p:p + ln].copy()
        kind = i % 5
        if kind == 1:
            s[int(rng.integers(0, ln))] = (s[int(rng.integers(0, ln))] + 1) % 4
        elif kind == 2:
            s = rng.integers(0, 4, ln).astype(np.uint8)
        elif kind == 3:
            s = _rc(s)
        ids = [[2, 4], [e + 1], [1], [2, 4, 1, 3]][i % 4]
        out.append((s, ids, int(rng.integers(0, 5))))
    out.append((np.zeros(30, np.uint8), [2, 4], 1))
    out.append((np.zeros(30, np.uint8), [1], 2))
    return out
