"""CBlitz's path stage (libkit4b/CBlitz.cpp) restated sequentially in Python (CPU): what `ngskit4b blitz` does with one query
between the nodes CSfxArray::LocateQuerySeqs returned (tests/query_ref.py) and its PSL line -- SortQueryAlignNodes (:3596), the
outer and the inner IdentifyHighScorePaths (:2603, :1641), HighScoreSW (:1560), ConsolidateNodes (:2157), CharacterisePath
(:2666), BlocksAlignStats (:1729), the automatic minimum score (:1539) and ReportAsPSL (:1925).  tests/test_blitz_cpu.py pins it
line for line to what the reference itself wrote (tests/golden/blitz_*.xz), so that the GPU tests may use it on fresh inputs
where the reference is absent.

HighScoreSW is recursive in the reference.  A successor s of a node c starts no earlier than c.start + c.len - 8 on the query
and on the target, and a node is at least core_len >= 8 long, so (s.qs, s.tl) >= (c.qs, c.tl) and s.qs + s.tl >= c.qs + c.tl:
the scores are filled here from the back of the sorted group, which is an order of falling-or-equal (qs, tl) and in which every
successor is scored before its predecessors.  Both properties are asserted for every successor met; `counters` (a dict) takes the
number of successors checked and of the branches the crafted cases are meant to reach.

An index is query_ref's (seq, sa, entries).  A path is a tuple in PATH_FIELDS order, its blocks a list of (len, q_start, t_start).
"""
import math

import numpy as np

PATH_FIELDS = ("query", "targ_seq_id", "strand", "score", "matches", "mismatches", "n_count", "q_num_insert", "q_base_insert",
               "t_num_insert", "t_base_insert", "q_start", "q_end", "t_start", "t_end", "n_blocks", "block_off")
BLOCK_FIELDS = ("len", "q_start", "t_start")
PARAM_NAMES = ("match_pts", "mismatch_pts", "gap_open", "min_path_score", "query_len_aligned_pct", "max_paths", "strand")
U32 = 0xFFFFFFFF
OVERLAP_FLOAT = 8     # cMaxBlitzOverlapFloat
MAX_GAP = 500000      # cGapBlitzMaxLength


class _Node:
    __slots__ = ("qs", "al", "tid", "tl", "mm", "fs", "rpt", "first", "scored", "hi", "nxt")

    def __init__(self, n):
        self.qs, self.al, self.tid, self.tl, self.mm, _, self.fs = (int(v) for v in n)
        self.rpt = self.first = self.scored = False
        self.hi = self.nxt = 0


def _bump(counters, key, by=1):
    if counters is not None:
        counters[key] = counters.get(key, 0) + by


def _own_score(nd, match, mismatch):
    s = nd.al * match
    if nd.mm:
        s = 0 if nd.mm * mismatch >= s else s - nd.mm * mismatch
    return s


def _score_group(grp, fs, match, mismatch, gap_open, counters):
    """HighScoreSW for every unflagged node of strand fs in the group, filled from the back"""
    for i in range(len(grp) - 1, -1, -1):
        c = grp[i]
        if c.rpt or c.fs != fs:
            continue
        own = _own_score(c, match, mismatch)
        c.hi, c.nxt = own, 0
        best = 0
        for j, s in enumerate(grp):
            if j == i or s.tid != c.tid or s.rpt or s.fs != fs:
                continue
            if s.tl < ((c.tl + c.al - OVERLAP_FLOAT) & U32) or s.tl > ((c.tl + c.al + MAX_GAP) & U32):
                continue
            if s.qs < ((c.qs + c.al - OVERLAP_FLOAT) & U32):
                if s.qs == c.qs + c.al - OVERLAP_FLOAT - 1:
                    _bump(counters, "overlap_9_rejected")
                continue
            # the fill order: the successor lies behind c in the sorted group and has been scored
            assert (s.qs, s.tl) > (c.qs, c.tl) and s.qs + s.tl >= c.qs + c.tl and j > i and s.scored, "HighScoreSW fill order"
            _bump(counters, "successors")
            qg, tg = s.qs - (c.qs + c.al), s.tl - (c.tl + c.al)
            if qg < 0 or tg < 0:
                _bump(counters, "overlap_%d" % max(-qg, -tg))
            gap_len = math.isqrt(qg * qg + tg * tg)
            if qg or tg:
                _bump(counters, "sqrt_exact" if gap_len * gap_len == qg * qg + tg * tg else "sqrt_floor")
            gap = min(1 + gap_len // 10, 10) + gap_open
            put = s.hi + own
            put = 0 if gap >= put else put - gap
            if put > best:
                best = put
                c.hi, c.nxt = best, j + 1
        c.scored = True


def _inner(nodes, start, count, fs, query_len, min_path_score, max_paths, pct, match, mismatch, gap_open, counters):
    """the inner IdentifyHighScorePaths (:1641-1725) over nodes[start : start + count]"""
    min_path_score = max(min_path_score, 25)
    grp = nodes[start:start + count]
    n_put = 0
    n_strand = sum(1 for nd in grp if nd.fs == fs)
    if n_strand > 64:
        _bump(counters, "group_over_128" if n_strand > 128 else "group_over_64")
    while True:
        for nd in grp:
            if nd.fs != fs or nd.rpt:
                continue
            nd.first = nd.rpt = nd.scored = False
            nd.hi = nd.nxt = 0
        _score_group(grp, fs, match, mismatch, gap_open, counters)
        best, best_i = 0, 0
        for i, nd in enumerate(grp):
            if nd.rpt or nd.fs != fs:
                continue
            if nd.hi > best:
                best, best_i = nd.hi, i + 1
        if best >= min_path_score:
            al, k = 0, best_i
            while k:
                al += grp[k - 1].al
                k = grp[k - 1].nxt
            if (al * 100) // query_len >= pct:
                k = best_i
                while k:
                    nd = grp[k - 1]
                    nd.first = k == best_i
                    nd.rpt = True
                    k = nd.nxt
                    if k:
                        nd.nxt = k + start
                n_put += 1
            else:
                _bump(counters, "pct_cut")
                best = 0
        if not (best >= min_path_score and n_put < max_paths):
            break
    return n_put


def _heads(nodes, query_len, min_path_score, max_paths, pct, strand, match, mismatch, gap_open, counters):
    """the outer IdentifyHighScorePaths (:2603-2663): the head nodes to report, in order"""
    n = len(nodes)
    cur_tid, cnt, start, n_put = nodes[0].tid, 0, 1, 0
    for end in range(1, n + 1):
        nd = nodes[end - 1]
        if nd.tid != cur_tid or end == n:
            if end == n:
                cnt += 1
                if nd.tid != cur_tid:
                    _bump(counters, "last_node_alone")
            for fs in (0, 1):
                if (fs == 0 and strand != 2) or (fs == 1 and strand != 1):
                    n_put += _inner(nodes, start - 1, cnt, fs, query_len, min_path_score, max_paths, pct, match, mismatch, gap_open, counters)
            cur_tid, cnt, start = nd.tid, 0, end
        cnt += 1
    if n_put == 0:
        return []
    heads = [i for i, nd in enumerate(nodes) if nd.first]
    keys = [(-nodes[i].hi, nodes[i].tid) for i in heads]
    kept = sorted(range(len(heads)), key=lambda k: keys[k])[:min(max_paths, len(heads))]
    if counters is not None:  # no kept head may tie with another head: qsort's order among equals is not defined
        for k in kept:
            assert keys.count(keys[k]) == 1, "tie among the heads"
    return [heads[k] for k in kept]


def _targ_base(index, ents, tid, loci):
    seq = index[0]
    start, seq_len = ents[tid]
    return seq[start + loci] & 0x0F if 0 <= loci < seq_len else 0xFF


def _consolidate(index, ents, nodes, head, q, counters):
    """ConsolidateNodes (:2157-2320); q is the query in the path's orientation"""
    cur = nodes[head]
    if cur.nxt == 0:
        return
    while cur.nxt != 0:
        nx = nodes[cur.nxt - 1]
        c_al, c_qs, c_tl = cur.al, cur.qs, cur.tl
        n_al, n_qs, n_tl = nx.al, nx.qs, nx.tl
        dq = n_qs - (c_qs + c_al - 1)
        dt = n_tl - (c_tl + c_al - 1)
        delta = dq if abs(dq) <= abs(dt) else dt
        if delta > 1:
            _bump(counters, "gap_closed_%d" % (delta - 1))
            cp, npos = c_qs + c_al, n_qs - 1
            ct, nt = c_tl + c_al, n_tl - 1
            while delta > 1:
                delta -= 1
                cb, nb = _targ_base(index, ents, cur.tid, ct), _targ_base(index, ents, nx.tid, nt)
                cm, nm = int(q[cp]) == cb, int(q[npos]) == nb
                if cm == nm:
                    _bump(counters, "gap_tie_odd" if delta & 1 else "gap_tie_even")
                    cm = bool(delta & 1)
                if cm:
                    c_al += 1
                    if int(q[cp]) != cb:
                        cur.mm += 1
                    ct += 1
                    cp += 1
                else:
                    n_al += 1
                    if int(q[npos]) != nb:
                        nx.mm += 1
                    n_qs -= 1
                    n_tl -= 1
                    nt -= 1
                    npos -= 1
        elif delta < 0:
            _bump(counters, "overlap_trimmed")
            cp, npos = c_qs + c_al - 1, n_qs
            ct, nt = c_tl + c_al - 1, n_tl
            while delta < 1:
                delta += 1
                cb, nb = _targ_base(index, ents, cur.tid, ct), _targ_base(index, ents, nx.tid, nt)
                cm, nm = int(q[cp]) == cb, int(q[npos]) == nb
                if cm == nm:
                    _bump(counters, "trim_tie_odd" if delta & 1 else "trim_tie_even")
                    nm = bool(delta & 1)
                if nm:
                    c_al -= 1
                    if int(q[cp]) != cb:
                        cur.mm -= 1
                    ct -= 1
                    cp -= 1
                else:
                    n_al -= 1
                    n_qs += 1
                    n_tl += 1
                    if int(q[npos]) != nb:
                        nx.mm -= 1
                    nt += 1
                    npos += 1
        elif delta == 0:
            # Delta == 0 is `Delta < 0 || Delta > 1` false: nothing is moved
            _bump(counters, "delta_zero")
        cur.al, cur.qs, cur.tl = c_al & U32, c_qs, c_tl
        nx.al, nx.qs, nx.tl = n_al & U32, n_qs & U32, n_tl & U32
        if cur.al == 0:
            _bump(counters, "zero_len_cur")
            cur.nxt, cur.al, cur.mm = nx.nxt, nx.al, nx.mm
            continue
        if nx.al == 0:
            _bump(counters, "zero_len_next")
            cur.nxt = nx.nxt
            continue
        if nx.qs - (cur.qs + cur.al - 1) == 1 and nx.tl - (cur.tl + cur.al - 1) == 1:
            _bump(counters, "coincident_merge")
            cur.nxt = nx.nxt
            cur.al += nx.al
            cur.mm += nx.mm
            continue
        cur = nx


def _characterise(nodes, head, counters):
    """CharacterisePath (:2666-2779): (q_end, t_end, q_num_insert, q_base_insert, t_num_insert, t_base_insert, n_nodes)"""
    h = nodes[head]
    q_end, t_end = h.qs + h.al - 1, h.tl + h.al - 1
    tt, qe, te = h, q_end, t_end
    while tt.nxt:
        tt = nodes[tt.nxt - 1]
        qg, tg = tt.qs - qe - 1, tt.tl - te - 1
        if qg < 0 or tg < 0:
            _bump(counters, "second_trim")
            d = -tg if qg >= 0 else (-qg if tg >= 0 else -min(qg, tg))
            tt.qs, tt.tl, tt.al = (tt.qs + d) & U32, (tt.tl + d) & U32, (tt.al - d) & U32
        qe, te = tt.qs + tt.al - 1, tt.tl + tt.al - 1
    qn = qb = tn = tb = 0
    n_nodes, cur = 1, h
    while cur.nxt:
        cur = nodes[cur.nxt - 1]
        qg, tg = cur.qs - q_end - 1, cur.tl - t_end - 1
        q_end, t_end = cur.qs + cur.al - 1, cur.tl + cur.al - 1
        if qg > 0:
            qn, qb = qn + 1, qb + qg
        if tg > 0:
            tn, tb = tn + 1, tb + tg
        n_nodes += 1
    return q_end & U32, t_end & U32, qn, qb & U32, tn, tb & U32, n_nodes


def _stats(index, ents, nodes, head, q, counters):
    """BlocksAlignStats (:1729-1849): (matches, mismatches, n_count)"""
    m = x = nn = 0
    cur = nodes[head]
    while True:
        for k in range(cur.al):
            qb, tb = int(q[cur.qs + k]), _targ_base(index, ents, cur.tid, cur.tl + k)
            if (qb & 7) > 3 or (tb & 7) > 3:
                nn += 1
                x += 1
            elif qb == tb:
                m += 1
            else:
                x += 1
        if not cur.nxt:
            break
        cur = nodes[cur.nxt - 1]
    if nn:
        _bump(counters, "n_in_block")
    return m, x, nn


def blitz_paths(index, query, nodes, match_pts=1, mismatch_pts=2, gap_open=5, min_path_score=0, query_len_aligned_pct=75, max_paths=1,
                strand=0, query_idx=0, counters=None):
    """one query with its LocateQuerySeqs nodes (query_ref.NODE_FIELDS tuples): ([path tuples], [block tuples]); block_off counts
    from this query's first block.  A query under 8 bases is shorter than any node and gets no path."""
    if len(nodes) == 0 or len(query) < 8:
        return [], []
    from query_ref import revcomp

    ents = {e[0]: (e[1], e[2]) for e in index[2]}
    qlen = len(query)
    fwd = np.asarray(query, dtype=np.uint8) & 0x0F
    rev = revcomp(fwd)
    ns = sorted((_Node(n) for n in nodes), key=lambda d: (d.tid, d.fs, d.qs, d.tl))
    if min_path_score > 0:
        mps = min_path_score
        if min_path_score < 25:
            _bump(counters, "min_score_floored")
    else:
        mps = ((qlen - 5) * match_pts) // 3
        _bump(counters, "min_score_auto")
    heads = _heads(ns, qlen, mps, max_paths, query_len_aligned_pct, strand, match_pts, mismatch_pts, gap_open, counters)
    paths, blocks = [], []
    for h in heads:
        hd = ns[h]
        q = rev if hd.fs else fwd
        if hd.fs:
            _bump(counters, "antisense_path")
        _consolidate(index, ents, ns, h, q, counters)
        q_end, t_end, qn, qb, tn, tb, n_nodes = _characterise(ns, h, counters)
        m, x, nn = _stats(index, ents, ns, h, q, counters)
        off = len(blocks)
        cur = hd
        while True:
            blocks.append((cur.al, cur.qs, cur.tl))
            if not cur.nxt:
                break
            cur = ns[cur.nxt - 1]
        assert len(blocks) - off == n_nodes
        _bump(counters, "blocks_%d" % min(n_nodes, 3))
        paths.append((query_idx, hd.tid, hd.fs, hd.hi, m, x, nn, qn, qb, tn, tb, hd.qs, q_end, hd.tl, t_end, n_nodes, off))
    return paths, blocks


def psl_line(name, query_len, targ_name, targ_len, path, blocks):
    """ReportAsPSL (:1925-2006) for one path tuple and its blocks, without the newline"""
    p = dict(zip(PATH_FIELDS, path))
    plus = p["strand"] == 0
    head = [p["matches"], p["mismatches"], 0, p["n_count"], p["q_num_insert"], p["q_base_insert"], p["t_num_insert"], p["t_base_insert"],
            "+" if plus else "-", name, query_len, p["q_start"] if plus else query_len - (p["q_end"] + 1),
            p["q_end"] + 1 if plus else query_len - p["q_start"], targ_name, targ_len, p["t_start"], p["t_end"] + 1, p["n_blocks"]]
    cols = [str(v) for v in head] + ["".join("%d," % b[k] for b in blocks) for k in range(3)]
    return "\t".join(cols)
