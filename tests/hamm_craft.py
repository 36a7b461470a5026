"""The seeded targets and crafted spans of the restricted-Hamming tests (numpy, CPU): tests/golden/make_golden_hamm.py runs the
reference over them, test_hamm_cpu.py the Python restatement, test_gpu_hamm.py the device.  K = 60 throughout: 60 / 7 = 8 leaves a
tail of 4 bases outside the segments of the last stage at rhamm 6.

targets(): h1 3000, h2 2000, h3 2500, h4 12000 (longer than the 10 000-base span cut of `ngskit4b hammings`)
cases():   [(name, form, what, params, expect)]; form "sfx": what = (entry_id, entry_loci, span_len); form "seq": what = a sequence.
           params = (rhamm, both_strands, sample_nth, min_core_depth, max_core_depth, intra_inter_both); expect = {offset in the
           span: byte} for the K-mers the case was made for (the restatement and the reference must agree with it), or None.
"""
import numpy as np

SEED = 0x48414D4D
K = 60
PARAM_NAMES = ("rhamm", "both_strands", "sample_nth", "min_core_depth", "max_core_depth", "intra_inter_both")
DEPTH_COPIES = 40


def _rng(*k):
    return np.random.default_rng([SEED, *k])


def revcomp(q):
    q = np.asarray(q, dtype=np.uint8)[::-1].copy()
    m = q <= 3
    q[m] = 3 - q[m]
    return q


def _mutate(s, positions):
    s = s.copy()
    for p in positions:
        s[p] = (s[p] + 1) % 4
    return s


def spread(d):
    """d substitutions, one in the middle of each of d equal parts of the K-mer: every segment of the stages before (d, d) holds one"""
    return [int((i + 0.5) * K / d) for i in range(d)]


# where things are: (entry index, locus) of the K-mer a case looks at
UNIQUE = (0, 100)
COPY_INTRA = (0, 200)       # copied to h1 1200
COPY_INTER = (0, 300)       # copied to h2 500
NEAR = {d: (0, 400 + 100 * d) for d in range(1, 7)}  # copy with d substitutions at h2 700 + 100 d
INTRA_NEAR = (0, 2000)      # copy with 1 substitution at h1 2300
BEFORE_START = (0, 1500)    # its second half is h1[0:30]
PAST_END = (0, 1600)        # its first half ends the last target
PALINDROME = (0, 2500)
REV_ONLY = (0, 2600)        # its reverse complement is at h3 100
DUP_SEG = (0, 2700)         # copy with 4 substitutions in the last quarter at h3 300
N_NEIGHBOUR = (0, 2800)     # copy with one N at h3 1800
EOS_CROSS = (0, 2900)       # its first half ends h2
N1, N2, N4, N5 = (2, 1000), (2, 1200), (2, 1400), (2, 1600)  # K-mers of h3 that start there hold 1, 2, 4, 5 N
N1_CLOSER = (2, 2000)       # a K-mer with 1 N whose substituted form is exact at h2 300
DEPTH_EARLY, DEPTH_LATE = (3, 6000), (3, 9000)  # K-mers of h4 whose first half is planted DEPTH_COPIES times


def targets():
    lens = (3000, 2000, 2500, 12000)
    h = [_rng(1, i).integers(0, 4, n).astype(np.uint8) for i, n in enumerate(lens)]
    h1, h2, h3, h4 = h
    h1[1200:1200 + K] = h1[200:200 + K]
    h2[500:500 + K] = h1[300:300 + K]
    for d in range(1, 7):
        s = NEAR[d][1]
        h2[700 + 100 * d:700 + 100 * d + K] = _mutate(h1[s:s + K], spread(d))
    h1[2300:2300 + K] = _mutate(h1[2000:2000 + K], [40])
    h1[1530:1560] = h1[0:30]
    x = _rng(2).integers(0, 4, K // 2).astype(np.uint8)
    h1[2500:2500 + K] = np.concatenate([x, revcomp(x)])
    h3[100:100 + K] = revcomp(h1[2600:2600 + K])
    h3[300:300 + K] = _mutate(h1[2700:2700 + K], [46, 50, 54, 58])
    h3[1800:1800 + K] = h1[2800:2800 + K]
    h3[1800 + 45] = 4
    h2[-30:] = h1[2900:2930]
    h3[1000 + 20] = 4
    h3[1200 + 20] = 4
    h3[1200 + 31] = 4
    for p in (10, 22, 35, 50):
        h3[1400 + p] = 4
    for p in (5, 15, 25, 35, 45):
        h3[1600 + p] = 4
    h3[2000:2000 + K] = h2[300:300 + K]
    h3[2000 + 33] = 4
    # depth: the first half of the K-mer DEPTH_COPIES times with fresh tails; the K-mer and its neighbour (1 substitution in the
    # second half) sort in front of (tails AAA..) or behind (tails TTT..) every planted copy
    for (_, at), lead, others, seed in ((DEPTH_EARLY, 0, (1, 2, 3), 3), (DEPTH_LATE, 3, (0, 1, 2), 4)):
        r = _rng(seed)
        core = r.integers(0, 4, K // 2).astype(np.uint8)
        tail = r.integers(0, 4, K // 2).astype(np.uint8)
        tail[:3] = lead
        h4[at:at + K] = np.concatenate([core, tail])
        h4[at + 100:at + 100 + K] = np.concatenate([core, _mutate(tail, [20])])
        for c in range(DEPTH_COPIES):
            p = at + 200 + 65 * c
            h4[p:p + K // 2] = core
            h4[p + K // 2] = others[c % 3]
    h4[-30:] = h1[1600:1630]
    return ["h%d" % (i + 1) for i in range(4)], h


def _p(rhamm=3, both=0, nth=1, mn=3, mx=4, iib=0):
    return (rhamm, both, nth, mn, mx, iib)


def cases():
    names, h = targets()
    out = []

    def one(name, at, expect, **kw):  # the span is the K-mer alone
        out.append((name, "sfx", (at[0] + 1, at[1], K), _p(**kw), {0: expect}))

    for r in range(1, 7):
        one("unique_r%d" % r, UNIQUE, r + 1, rhamm=r)  # the last stage's ProbeLen / CoreLen
    for iib, a, b in ((0, 0, 0), (1, 0, 4), (2, 4, 0)):
        one("copy_intra_z%d" % iib, COPY_INTRA, a, iib=iib)
        one("copy_inter_z%d" % iib, COPY_INTER, b, iib=iib)
    one("palindrome_sense", PALINDROME, 4)
    one("palindrome_both", PALINDROME, 0, both=1)
    one("rev_only_sense", REV_ONLY, 4)
    one("rev_only_both", REV_ONLY, 0, both=1)
    for d in range(1, 7):
        one("near%d" % d, NEAR[d], d, rhamm=6)
        if d > 1:
            one("near%d_r%d" % (d, d - 1), NEAR[d], d, rhamm=d - 1)  # the stage before misses it and answers its own ProbeLen / CoreLen
    one("near1_z1", NEAR[1], 1, iib=1)       # an inexact neighbour in the other entry under `intra only`: still counted
    one("intra_near_z2", INTRA_NEAR, 1, iib=2)  # ... in the same entry under `inter only`
    one("dup_segment", DUP_SEG, 4, rhamm=4)
    one("n_in_neighbour", N_NEIGHBOUR, 1)
    one("eos_cross", EOS_CROSS, 4)
    one("before_start", BEFORE_START, 4)
    one("past_end", PAST_END, 4)
    one("n1", (N1[0], N1[1]), 1)
    one("n2", (N2[0], N2[1]), 2)
    one("n4", (N4[0], N4[1]), 4, rhamm=4)
    one("n5", (N5[0], N5[1]), 0)
    one("n1_closer", N1_CLOSER, 0)
    # depth caps (rhamm 1: only the (0,1) stage, whose depths are 2 x min / 10 x max): 42 occurrences of the first half
    one("depth_inside", DEPTH_EARLY, 1, rhamm=1, mn=0, mx=2)     # 20 of 42 explored, the neighbour among them
    one("depth_beyond", DEPTH_LATE, 2, rhamm=1, mn=0, mx=2)      # ... the neighbour behind them
    one("depth_all", DEPTH_LATE, 1, rhamm=1, mn=0, mx=5)         # 50 >= 42: found
    one("depth_abandoned", DEPTH_LATE, 2, rhamm=1, mn=2, mx=2)   # counted on the 4th turn: 41 > 20, given up
    one("depth_abandoned_early", DEPTH_EARLY, 1, rhamm=1, mn=2, mx=2)  # ... after the neighbour was met
    # spans
    out.append(("span_h1_head", "sfx", (1, 0, 500), _p(rhamm=2), None))
    out.append(("span_nth3", "sfx", (1, 150, 400), _p(rhamm=2, nth=3), None))
    out.append(("span_h3_ns_both", "sfx", (3, 960, 750), _p(rhamm=3, both=1), None))
    out.append(("span_h2_tail", "sfx", (2, 2000 - 150, 150), _p(rhamm=6), None))
    # the LocateHammings form: outside sequences
    q = np.concatenate([h[0][180:330], _mutate(h[1][1000:1090], [10, 70]), _rng(9).integers(0, 4, 80).astype(np.uint8)])
    qn = q.copy()
    qn[[30, 200]] = 4
    out.append(("seq_outside", "seq", q, _p(rhamm=3), None))
    out.append(("seq_outside_n_both_nth2", "seq", qn, _p(rhamm=3, both=1, nth=2), None))
    out.append(("seq_one_kmer", "seq", h[0][200:200 + K].copy(), _p(rhamm=2), {0: 0}))  # (no self hit to skip: ProbeEntry 0)
    return out


CSV_RUNS = (("hamm_k60_r3", dict(kmer_len=60, rhamm=3)), ("hamm_k60_r2_k3_c", dict(kmer_len=60, rhamm=2, sample_nth=3, both_strands=True)),
            ("hamm_k100_r3_z2", dict(kmer_len=100, rhamm=3, intra_inter_both=2)))
