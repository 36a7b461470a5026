"""A crafted index and the cases for `genzygosity` and CSfxArray::LocateAllNearMatches under it (tests/zyg_ref.py restates them,
tests/golden/make_golden_zygosity.py records the reference, test_zygosity_cpu.py and test_gpu_zygosity.py compare).

Eight entries of 2000 to 3300 bases.  sites() tells where each planted site stands and what it was made for.
  sisters    zB and zC are zA with 1 % and 4 % of the bases substituted: foreign matches at 0, 1, 2 and 3 mismatches
  dup/dup1   a 30-mer twice in zD, exact and with one base changed; rcdup: its reverse complement again in zD
  pal        a 50-base reverse palindrome in zD: every centred even window is its own minus-strand hit at its own locus
  sep        a 30-mer of zD whose first half ends zE and whose second half begins zF: the core hit runs across the separator
  nruns      N runs of 1, 2 and 6 in zE
  head/tail  the second core of a zD window again in the first bases of zA (the hit's left end would lie in front of the
             concatenation), the first core of another again in the last bases of zH (its right end behind it)
  fam        one 30-mer in zD, zE, zF, zG and zH: four foreign hits, more than -x3 allows
  ac / ag    (AC)n in zE..zH, 1220 copies of either 11-mer: a run the check at the 100th iteration gives up on at MaxIter 1000;
             (AG)n in zE..zG, 1050 copies: a run that is walked until MaxIter 1000 cuts it
  acp / agp  zD windows of 14 random bases and 11 of (AC)n / (AG)n: unique probes whose last core meets those runs
  per        UUV in zD and zE with U of 9 bases: the cores at 0 and 9 are the same, the dedupe decides the count
"""
import numpy as np

N_ = 4
NAMES = ["zA", "zB", "zC", "zD", "zE", "zF", "zG", "zH"]


def _rc(a):
    a = np.asarray(a, dtype=np.uint8)[::-1].copy()
    m = a <= 3
    a[m] = 3 - a[m]
    return a


def build():
    """(names, sequences, sites): sites[name] = (entry id, locus) of the site's first base"""
    rng = np.random.default_rng(30311)

    def rnd(n):
        return rng.integers(0, 4, n).astype(np.uint8)

    def sister(a, rate):
        b = a.copy()
        at = rng.choice(len(a), int(len(a) * rate), replace=False)
        b[at] = (b[at] + rng.integers(1, 4, len(at))) % 4
        return b

    parts = {n: [] for n in NAMES}
    sites = {}

    def put(name, *chunks, site=None):
        if site:
            sites[site] = (NAMES.index(name) + 1, sum(len(c) for c in parts[name]))
        parts[name].extend(np.asarray(c, dtype=np.uint8) for c in chunks)

    m = {k: rnd(30) for k in ("dup", "sep", "head", "tail", "fam")}
    dup1 = m["dup"].copy()
    dup1[17] = (dup1[17] + 1) % 4
    half = rnd(25)
    u, v = rnd(9), rnd(7)
    ac = np.tile(np.array([0, 1], np.uint8), 310)  # 620 bases: 305 copies of either 11-mer
    ag = np.tile(np.array([0, 2], np.uint8), 355)  # 710 bases: 350 copies
    n = lambda k: np.full(k, N_, np.uint8)

    put("zA", rnd(3), m["head"][9:18], site="head_core")  # bases 3..11 of the concatenation: as core 9 of `head` the left end is at -6
    base = rnd(2000)
    put("zA", base, site="base")
    put("zB", rnd(9), sister(base, 0.01))
    put("zC", rnd(9), sister(base, 0.04))
    put("zD", rnd(100))
    for k, s in (("dup", m["dup"]), ("dup1", dup1), ("rcdup", _rc(m["dup"])), ("dup_again", m["dup"]), ("pal", np.concatenate([half, _rc(half)])),
                 ("sep", m["sep"]), ("head", m["head"]), ("tail", m["tail"]), ("fam", m["fam"]), ("per", np.concatenate([u, u, v])),
                 ("acp", np.concatenate([rnd(14), ac[:11]])), ("agp", np.concatenate([rnd(14), ag[:11]])),
                 ("acp50", np.concatenate([rnd(40), ac[:10]]))):
        put("zD", s, site=k)
        put("zD", rnd(70))
    put("zD", rnd(900))
    put("zE", rnd(200))
    for k in (1, 2, 6):
        put("zE", n(k), rnd(60), site="nrun%d" % k)
    put("zE", np.concatenate([u, u, v]), rnd(50), site="per_e")
    for name in ("zE", "zF", "zG", "zH"):
        put(name, rnd(150), m["fam"], rnd(100), ac, rnd(300))
    for name in ("zE", "zF", "zG"):
        put(name, ag, rnd(200))
    put("zH", rnd(800))
    put("zE", rnd(40), m["sep"][:15])       # ... | separator | ...
    parts["zF"].insert(0, m["sep"][15:])
    put("zF", rnd(120))
    put("zG", rnd(120))
    put("zH", rnd(60), m["tail"][:9], rnd(5), site="tail_pre")  # the core 14 bases before the end: 25 from its left end pass it
    seqs = [np.concatenate(parts[k]) for k in NAMES]
    return NAMES, seqs, sites


def short_entry():
    """three entries, the middle one of 22 bases: shorter than -l25: no source windows, and no window of the others fits into it"""
    rng = np.random.default_rng(30312)
    a = rng.integers(0, 4, 400).astype(np.uint8)
    return ["s1", "tiny", "s3"], [a, a[100:122].copy(), np.concatenate([rng.integers(0, 4, 50).astype(np.uint8), a[90:140]])]


def scan_cases():
    """(file stem, kwargs of zygosity / genzygosity_csv): the four recorded runs of `genzygosity`"""
    return [("zygosity_l25_s2", dict(subseq_len=25, max_subs=2)),
            ("zygosity_l25_s2_m3_x3", dict(subseq_len=25, max_subs=2, mode=3, max_matches=3)),
            ("zygosity_l50_s4_n5_m2", dict(subseq_len=50, max_subs=4, max_ns=5, mode=2)),
            ("zygosity_l20_s0_n0_z001", dict(subseq_len=20, max_subs=0, max_ns=0, threshold=0.01))]


def front_end_args(kw):
    a = ["-l%d" % kw["subseq_len"], "-s%d" % kw["max_subs"]]
    for k, f in (("max_ns", "-n%d"), ("mode", "-m%d"), ("max_matches", "-x%d"), ("threshold", "-z%g")):
        if k in kw:
            a.append(f % kw[k])
    return a


def error_cases():
    """kwargs of zygosity that give K4_ERR_PARAMS"""
    return [dict(subseq_len=19), dict(subseq_len=1001), dict(subseq_len=25, max_subs=8), dict(max_subs=-1), dict(max_ns=6), dict(max_ns=-1),
            dict(max_matches=-1), dict(max_matches=1000001), dict(mode=4), dict(mode=-1), dict(src_first=0), dict(src_first=9),
            dict(src_first=8, src_count=2), dict(src_count=-1)]


def near_error_cases():
    """(probe length, kwargs of all_near_matches) that give K4_ERR_PARAMS"""
    ok = dict(max_tot_mm=2, core_len=9, core_delta=9, max_core_slides=4)
    return [(1001, ok), (25, dict(ok, core_len=0)), (25, dict(ok, core_len=26)), (25, dict(ok, core_delta=0)), (25, dict(ok, max_core_slides=0)),
            (25, dict(ok, max_core_slides=33)), (25, dict(ok, max_tot_mm=-1)), (25, dict(ok, max_matches=-1)), (25, dict(ok, cur_max_iter=-1)),
            (25, dict(ok, n_ident_nodes=-1))]


def calls(seqs, sites):
    """the LocateAllNearMatches calls that were recorded: dicts with probe, probe_entry, probe_ofs, num_entries and the limits.
    Windows at and around every site, of 25, 50 and 20 bases, then random windows; MaxMatches 0 / 1 / 3, CurMaxIter 0 / 50 / 1000,
    ident nodes 3 / 40 / 1 024 000, NumEntries 8 / 5 / 0, slides 1 / 3 / 8 -- each cycled at its own pace."""
    rng = np.random.default_rng(30313)
    out = []

    def add(e, ofs, ln, k):
        if ofs < 0 or ofs + ln > len(seqs[e - 1]):
            return
        mm, cl = ((2, 9), (4, 10), (0, 20), (2, 11), (3, 6))[k % 5] if ln != 50 else ((4, 10), (2, 16))[k % 2]
        if ln == 20:
            mm, cl = ((0, 20), (1, 10))[k % 2]
        out.append(dict(probe=seqs[e - 1][ofs:ofs + ln].copy(), probe_entry=e, probe_ofs=ofs, max_tot_mm=mm, core_len=cl,
                        core_delta=cl if k % 7 else max(1, cl // 2), max_core_slides=(8, 3, 1, 4)[k % 4], max_matches=(0, 0, 3, 1, 5000)[k % 5],
                        num_entries=(8, 8, 5, 8, 0, 8)[k % 6], cur_max_iter=(0, 1000, 50, 5000, 1000)[(k // 2) % 5],
                        n_ident_nodes=(1024000, 1024000, 40, 1024000, 3, 1024000, 1024000)[(k // 3) % 7]))

    k = 0
    for name, (e, at) in sorted(sites.items()):
        for ln in (25, 50, 20):
            for d in (0, 3, -4, 5, 11):
                add(e, at + d, ln, k)
                k += 1
    # the repeat families from a unique probe, with every limit that cuts them
    for name in ("acp", "agp"):
        e, at = sites[name]
        for it in (0, 50, 1000, 1100, 5000):
            for nodes in (1024000, 40, 900):
                out.append(dict(probe=seqs[e - 1][at:at + 25].copy(), probe_entry=e, probe_ofs=at, max_tot_mm=2, core_len=11, core_delta=11,
                                max_core_slides=3, max_matches=0, num_entries=8, cur_max_iter=it, n_ident_nodes=nodes))
    for name in ("acp", "agp"):  # shorter cores: the last one is right-aligned and still inside the family
        e, at = sites[name]
        for cl in (10, 9, 8, 7, 6):
            for it in (50, 100, 1000):
                out.append(dict(probe=seqs[e - 1][at:at + 25].copy(), probe_entry=e, probe_ofs=at, max_tot_mm=3, core_len=cl, core_delta=cl,
                                max_core_slides=8, max_matches=0, num_entries=8, cur_max_iter=it, n_ident_nodes=1024000))
    e, at = sites["fam"]  # four foreign hits against MaxMatches 1 and 3
    for d in range(6):
        for mx in (1, 3):
            out.append(dict(probe=seqs[e - 1][at + d:at + d + 25].copy(), probe_entry=e, probe_ofs=at + d, max_tot_mm=2, core_len=9, core_delta=9,
                            max_core_slides=4, max_matches=mx, num_entries=8, cur_max_iter=5000, n_ident_nodes=1024000))
    e, at = sites["acp50"]  # five cores of 10 over 50 bases around the site's random stretch
    for it in (1000, 0):
        out.append(dict(probe=seqs[e - 1][at - 20:at + 30].copy(), probe_entry=e, probe_ofs=at - 20, max_tot_mm=4, core_len=10, core_delta=10,
                        max_core_slides=8, max_matches=0, num_entries=8, cur_max_iter=it, n_ident_nodes=1024000))
    # a window of a sister entry asked as if it came from elsewhere (its own place is then a foreign or an own-entry hit)
    for i in range(40):
        add(1 + i % 3, 100 + 37 * i, 25, k)
        out[-1]["probe_ofs"] += i % 2
        k += 1
    while len(out) < 480:
        e = int(rng.integers(1, len(seqs) + 1))
        ln = (25, 50, 20)[k % 3]
        add(e, int(rng.integers(0, len(seqs[e - 1]) - ln + 1)), ln, k)
        k += 1
    return out
