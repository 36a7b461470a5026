"""The crafted queries of the blitz path-stage tests (numpy, CPU), over tests/query_craft.py's targets and
tests/golden/query_index.sfx.xz: tests/golden/make_golden_blitz.py runs `ngskit4b blitz` over them, test_blitz_cpu.py the Python
restatement (tests/blitz_ref.py), test_gpu_blitz.py the device.

groups(): {group: (locate params, path params, [(case name, query)])} -- one reference run per group.  The locate params are
query_craft.PARAM_NAMES (core_len 20: above cMaxKmerLen, so blitz does not classify over-occurring K-mers; max_iter 100 is -k100;
max_hits 200 000 is cNumBlitzAllocdAlignNodes), the path params blitz_ref.PARAM_NAMES.  Every query is at least 100 bases, the
reference's shortest.  WANT: the branch counters of blitz_ref that each group has to reach.  unlinked(): hand-made nodes for the one
branch no group reaches, a block trimmed to zero length.

Junk that must stop an extension is not random: _avoid() picks, base by base, a base that differs from the target on both sides.
"""
import lzma
import os

import numpy as np

import query_craft as qc

LOCATE = qc._p(core_len=20, core_delta=10, max_hits=200000, max_iter=100, match_pts=1, mismatch_pts=2)


def _path(**kw):
    p = dict(match_pts=1, mismatch_pts=2, gap_open=5, min_path_score=0, query_len_aligned_pct=75, max_paths=1, strand=0)
    p.update(kw)
    return tuple(p[k] for k in ("match_pts", "mismatch_pts", "gap_open", "min_path_score", "query_len_aligned_pct", "max_paths", "strand"))


def _avoid(*segs):
    """a base per position that differs from every segment's base there"""
    n = len(segs[0])
    out = np.zeros(n, np.uint8)
    for k in range(n):
        used = {int(s[k]) for s in segs}
        out[k] = min(b for b in range(4) if b not in used)
    return out


def _extra(q, t, clean, cl=20, mp=1, xp=2):
    """LocateQuerySeqs's flank extension (query_ref.py) over the aligned bases q against t that follow `clean` matching ones: how
    far beyond the clean ones the reported flank reaches"""
    score = (cl + clean) * mp
    hi_score, hi_len, floor, mm = score, clean, score - 4 * mp, 0
    for k in range(min(len(q), len(t))):
        if q[k] > 3 or t[k] > 3 or q[k] != t[k]:
            score = max(score - xp, floor) if score > floor else floor
            mm += 1
        else:
            score += mp
        fl = clean + k + 1
        if score >= hi_score and (mm * 100) // (fl + cl) <= 15:
            hi_score, hi_len, floor = score, fl, score - 4 * mp
    return hi_len - clean


def _joint_is_exact(t, q, a, la, qb, b):
    """the node of t[a : a + la] at the query's start ends at la, the node of t[b :] at query offset qb starts there"""
    c0 = -(-qb // 10) * 10  # the first core inside the second piece
    back = q[:qb][::-1]
    return _extra(q[la:], t[a + la:], la - 20) == 0 and _extra(back, t[max(b - qb, 0):b][::-1], c0 - qb) == 0


def _gap(t, a, la, qgap, tgap, lb):
    """t[a : a + la], qgap bases that match neither side, t[a + la + tgap : .. + lb], for the first a at or behind the given one
    at which the two nodes come out with exactly that gap between them"""
    for a in range(a, len(t) - la - tgap - lb - 5):
        b = a + la + tgap
        junk = _avoid(t[a + la:a + la + qgap], t[b - qgap:b]) if qgap else np.zeros(0, np.uint8)
        q = np.concatenate([t[a:a + la], junk, t[b:b + lb]])
        if _joint_is_exact(t, q, a, la, la + qgap, b):
            return q
    raise AssertionError("no exact joint")


def _overlap_pair(t, k, length=120):
    """the query of t[a : a + length], which ends in the k bases t[b : b + length] starts with, and the rest of the latter, b
    behind a + length: two nodes over-extended into one another by exactly k"""
    n = len(t)
    for a in range(200, n - 2 * length - 200):
        e = a + length
        for b in range(e + 50, n - length - 10):
            if np.array_equal(t[e - k:e], t[b:b + k]):
                q = np.concatenate([t[a:e], t[b + k:b + length]])
                c0 = -(-(length - k) // 10) * 10
                if c0 - (length - k) >= k and _extra(q[length:], t[e:], length - 20) == 0 and \
                   _extra(q[:length - k][::-1], t[b - (length - k):b][::-1], c0 - (length - k)) == 0:
                    return q
    raise AssertionError("no %d-base overlap pair" % k)


def _three(t, a):
    """150 bases, 30 inserted, 150 bases, 30 deleted, 150 bases: three nodes"""
    two = _gap(t, a, 150, 30, 0, 150)
    a = next(x for x in range(a, len(t)) if np.array_equal(t[x:x + 150], two[:150]))
    return np.concatenate([two, t[a + 330:a + 480]])


def _scatter(t, n, seed):
    """n pieces of 30 bases from every 40th locus of t in a shuffled order: n nodes of one target and strand, chained wherever
    the loci rise along the query"""
    order = qc._rng(seed).permutation(n)
    return np.concatenate([t[40 * int(k) + 5:40 * int(k) + 35] for k in order])


def groups():
    _, ts = qc.targets()
    t1, t2, t3, t4, t5, t6, t7 = ts
    g = {}
    # -- one default run: indels, square roots, overlaps, closed gaps, merge, antisense, N
    c = [("exact400", t1[1000:1400])]
    c.append(("del30", _gap(t1, 2000, 200, 0, 30, 200)))
    c.append(("ins30", _gap(t1, 2000, 200, 30, 0, 200)))
    c.append(("ins30_del30", _three(t1, 2600)))
    c.append(("gap30_40", _gap(t1, 3200, 150, 30, 40, 150)))
    c.append(("gap30_39", _gap(t1, 3200, 150, 30, 39, 150)))
    for k in (1, 8, 9):
        c.append(("overlap%d" % k, _overlap_pair(t1, k)))
    for gq in (2, 7):
        c.append(("close%d" % gq, _gap(t4, 150 * gq, 150, gq, gq + 30, 150)))
    c.append(("merge20", _gap(t1, 4600, 45, 20, 20, 45)))
    c.append(("del30_rc", qc.revcomp(_gap(t1, 2000, 200, 0, 30, 200))))
    c.append(("close7_rc", qc.revcomp(_gap(t3, 600, 150, 7, 37, 150))))
    qn = _gap(t1, 5000, 150, 0, 30, 150).copy()
    qn[60] = 4
    c.append(("n_in_block", qn))
    c.append(("n_in_target", t2[1850:2150]))
    g["default"] = (LOCATE, _path(), c)
    # -- several targets and strands: each piece is a path of its own
    multi = np.concatenate([t1[1000:1200], qc.revcomp(t3[500:650]), t4[100:230], qc.revcomp(t1[3000:3110]), _gap(t3, 1500, 110, 0, 30, 110)])
    c = [("multi", multi), ("multi_rc", qc.revcomp(multi))]
    g["paths1"] = (LOCATE, _path(query_len_aligned_pct=10, min_path_score=25, max_paths=1), c)
    g["paths3"] = (LOCATE, _path(query_len_aligned_pct=10, min_path_score=25, max_paths=3), c)
    g["paths3_plus"] = (LOCATE, _path(query_len_aligned_pct=10, min_path_score=25, max_paths=3, strand=1), c)
    g["paths3_minus"] = (LOCATE, _path(query_len_aligned_pct=10, min_path_score=25, max_paths=3, strand=2), c)
    # -- the aligned-percentage cut: the best path of the group (150 clean bases, 37 %) fails it, the lesser one (210 bases with
    # seven substitutions at 10 points each, 52 %) would pass and is reported when it stands alone
    lesser = qc._sub(t1[3000:3210], list(range(25, 210, 30)))
    c = [("best_fails", np.concatenate([lesser, _avoid(t1[3210:3230], t1[980:1000]), t1[1000:1150], _avoid(t1[1150:1170], t1[3380:3400])])),
         ("lesser_alone", np.concatenate([lesser, _avoid(t1[3210:3400], t1[1000:1190])]))]
    g["pct_cut"] = (qc._p(core_len=20, core_delta=10, max_hits=200000, max_iter=100, match_pts=1, mismatch_pts=10),
                    _path(mismatch_pts=10, query_len_aligned_pct=50, min_path_score=25), c)
    # -- the last node alone on a new target; groups of more than 64 and more than 128 nodes (the wave width once and twice); a
    # different scoring
    c = [("last_alone", np.concatenate([_gap(t1, 2000, 150, 0, 30, 150), _avoid(t1[2330:2350], t7[6500:6520]), t7[6500:6540]])),
         ("scatter70", _scatter(t1, 70, 51)),
         ("scatter135", _scatter(t1, 135, 52)),
         ("tandem", np.concatenate([qc._junk(30, 25), t6[400:548], qc._junk(30, 26)]))]
    g["groups"] = (qc._p(core_len=20, core_delta=10, max_hits=200000, max_iter=100, match_pts=2, mismatch_pts=3),
                   _path(match_pts=2, mismatch_pts=3, gap_open=2, query_len_aligned_pct=10, min_path_score=25, max_paths=1), c)
    return g


# the counters of blitz_ref each group has to reach (test_blitz_cpu.py and the generator assert each is non-zero)
WANT = {
    "default": ("blocks_1", "blocks_2", "blocks_3", "sqrt_exact", "sqrt_floor", "overlap_1", "overlap_8", "overlap_9_rejected",
                "gap_closed_2", "gap_closed_7", "gap_closed_20", "gap_tie_odd", "gap_tie_even", "coincident_merge", "antisense_path",
                "n_in_block", "min_score_auto", "overlap_trimmed", "trim_tie_odd", "trim_tie_even"),
    "paths1": ("antisense_path",),
    "paths3": ("antisense_path", "blocks_2"),
    "paths3_plus": ("blocks_1",),
    "paths3_minus": ("antisense_path",),
    "pct_cut": ("pct_cut",),
    "groups": ("last_node_alone", "group_over_64", "group_over_128"),
}


GROUPS = tuple(WANT)


def golden_lines(golden_dir, group):
    """the PSL lines the reference wrote for the group (tests/golden/blitz_<group>.xz)"""
    with lzma.open(os.path.join(golden_dir, "blitz_%s.xz" % group), "rt") as f:
        return f.read().splitlines()


def _differs(t, at, seg):
    """the first place at or behind `at` where t differs from seg in every base"""
    return next(m for m in range(at, len(t) - len(seg)) if not np.any(t[m:m + len(seg)] == seg))


def unlinked():
    """Nodes made by hand, not found by LocateQuerySeqs, so that ConsolidateNodes' overlap trim consumes a whole node and unlinks it
    (:2291-2303): [(case name, query, [node tuples in query_ref.NODE_FIELDS order])], path params, {case: the blitz_ref counter
    it has to reach}.  No reference line exists for them: the device is compared with the restatement.

    Every query is 80 bases of the first target, A = t[a : a + 40] then B = t[b : b + 40]; node A covers the first half exactly,
    node B the second.  Between them stands a node M that claims to align, without mismatch, query bases that differ from its
    target bases everywhere, and that overlaps A by 8 bases:
      zero_next  M is 8 bases.  A's last base matches and M's never do, so all 8 trims fall on M as the next node.
      zero_cur   M is 16 bases and B overlaps it by 8.  The trim against A leaves it 8; against B, whose first base matches while
                 M's never do, all 8 fall on M as the current node, which then takes over B's length but keeps its own start.
      zero_cur_rc  the same on the antisense strand: the query reverse-complemented, the nodes on strand 1.
    The scores (match 3, gap open 1) make A -> M -> B beat A -> B."""
    _, ts = qc.targets()
    t, a = ts[0], 1000
    m = _differs(t, a + 100, t[a + 32:a + 40])                 # M's bases differ from the query's [32, 40)
    b8 = m + 50
    q8 = np.concatenate([t[a:a + 40], t[b8:b8 + 40]])
    b16 = _differs(t, m + 60, t[m + 8:m + 16])                 # and, where M is 16 long, from B's first 8
    q16 = np.concatenate([t[a:a + 40], t[b16:b16 + 40]])

    def nodes(m_len, b, fs):  # (query_start, align_len, targ_seq_id, targ_loci, n_mismatches, slot, strand)
        return [(0, 40, 1, a, 0, 0, fs), (32, m_len, 1, m, 0, 0, fs), (40, 40, 1, b, 0, 0, fs)]

    cases = [("zero_next", q8, nodes(8, b8, 0)), ("zero_cur", q16, nodes(16, b16, 0)), ("zero_cur_rc", qc.revcomp(q16), nodes(16, b16, 1))]
    want = {"zero_next": "zero_len_next", "zero_cur": "zero_len_cur", "zero_cur_rc": "zero_len_cur"}
    return cases, _path(match_pts=3, mismatch_pts=2, gap_open=1, min_path_score=25, query_len_aligned_pct=10), want


def mixed_batch():
    """0 to 5000 bases in one batch, with queries that have no node (at the start, in the middle and at the end) and queries whose
    nodes make no path: (queries, locate params, path params)"""
    _, ts = qc.targets()
    t1 = ts[0]
    r = qc._rng(31)
    cat = np.concatenate(ts)
    qs = [np.zeros(0, np.uint8), qc._junk(150, 41)]
    for k, ln in enumerate((100, 333, 64, 1000, 2500, 5000)):
        s = int(r.integers(0, len(ts[0]) - ln)) if ln <= 5000 else 0
        q = (t1 if ln < 5000 else cat)[s:s + ln].copy()
        pos = r.choice(ln, size=ln // 50, replace=False)
        q[pos] = (q[pos] + 1 + r.integers(0, 3, len(pos))) % 4
        qs.append(qc.revcomp(q) if k % 2 else q)
        if k == 2:
            qs.append(qc._junk(120, 42))                                     # no node, in the middle
            qs.append(np.concatenate([t1[500:530], qc._junk(170, 43)]))   # one node of 30 bases: under the minimum score
    qs.append(_gap(t1, 2000, 200, 12, 30, 200))
    qs.append(qc._junk(101, 44))
    return qs, LOCATE, _path(max_paths=2, query_len_aligned_pct=50)
