"""CSfxArray::LocateQuerySeqs (libkit4b/SfxArray.cpp:6493-6833) and NumExactKMers (:8122-8224) restated literally and
sequentially in Python (CPU): what the reference does with one query, step by step, in its own order.  tests/test_query_cpu.py
pins it node for node to what the reference itself returned (tests/golden/query_*.xz), so that the GPU tests may use it on
fresh inputs where the reference is absent.

An index is (seq, sa, entries): the concatenated sequence (codes 0..4, 7 behind every target), its suffix array as int64, and
[(entry_id, start_ofs, seq_len)] sorted by start.  Nodes are tuples in NODE_FIELDS order.
"""
import bisect

import numpy as np

NODE_FIELDS = ("query_start", "align_len", "targ_seq_id", "targ_loci", "n_mismatches", "slot", "strand")
U32 = 0xFFFFFFFF


def revcomp(q):
    q = np.asarray(q, dtype=np.uint8)[::-1].copy()
    m = q <= 3
    q[m] = 3 - q[m]
    return q


def _cmp(core, seq, pos):
    """CmpProbeTarg (:2508-2525)"""
    for j, p in enumerate(core):
        t = seq[pos + j] & 0x0F if pos + j < len(seq) else 7
        if t == 7:
            return -1
        if p != t:
            return 1 if p > t else -1
    return 0


def num_exact_kmers(index, core, max_to_match):
    """(first suffix-array index, count): the count is exact up to max_to_match and otherwise at least max_to_match + 1"""
    seq, sa, _ = index
    lo, hi = 0, len(sa)
    while lo < hi:
        mid = (lo + hi) // 2
        if _cmp(core, seq, int(sa[mid])) > 0:
            lo = mid + 1
        else:
            hi = mid
    first = lo
    n = 0
    while first + n < len(sa) and n <= max_to_match and _cmp(core, seq, int(sa[first + n])) == 0:
        n += 1
    return first, n


def locate_query_seqs(index, query, core_len, core_delta, strand=0, max_hits=1000, max_iter=100, match_pts=1, mismatch_pts=3):
    seq, sa, entries = index
    starts = [e[1] for e in entries]
    probe_len = len(query)
    hits = []  # dicts; index + 1 is the reference's node index
    targ_hash = [0] * 256
    num = 0
    fwd = [int(b) & 0x0F for b in query]
    rev = [int(b) for b in revcomp(fwd)]
    order = {0: ("+", "-"), 1: ("+",), 2: ("-",), 3: ("+",)}[strand]
    stop = False
    for cur_strand in order:
        if stop:
            break
        probe = fwd if cur_strand == "+" else rev
        fs = 0 if cur_strand == "+" else 1
        cur_delta = core_delta
        ofs = 0
        while ofs < ((probe_len - core_len) & U32) and probe_len > core_len:  # (a shorter query reads past its end in the reference)
            this_ofs = ofs
            if ((ofs + core_len + cur_delta) & U32) > probe_len:
                cur_delta = probe_len - (ofs + core_len)
            ofs += cur_delta
            core = probe[this_ofs:this_ofs + core_len]
            first, copies = num_exact_kmers(index, core, max_iter)
            if copies == 0 or copies >= max_iter:
                continue
            for it in range(copies):
                left = int(sa[first + it])
                e = bisect.bisect_right(starts, left) - 1
                targ_id, e_start, seq_len = entries[e]
                loci = left - e_start
                hidx = ((targ_id & 0x7F) << 1) | fs
                # containment (:6605-6623)
                si = targ_hash[hidx]
                contained = False
                while si != 0:
                    h = hits[si - 1]
                    if h["tid"] == targ_id:
                        if not (this_ofs < h["qs"] or this_ofs + core_len > h["qs"] + h["al"]) and \
                           not (loci < h["tl"] or loci + core_len > h["tl"] + h["al"]) and (this_ofs - h["qs"]) == (loci - h["tl"]):
                            contained = True
                            break
                    si = h["nxt"]
                if contained:
                    continue
                # 5' extension (:6628-6673)
                mm5 = 0
                score = core_len * match_pts
                floor = score - 4 * match_pts
                hi_score, hi_len, hi_mm = score, 0, 0
                fl = 0
                for k in range(min(loci, this_ofs)):
                    tb = seq[left - 1 - k] & 0x07
                    pb = probe[this_ofs - 1 - k] & 0x07
                    if tb > 4 or pb > 4:
                        break
                    if tb == 4 or pb == 4 or pb != tb:
                        if score >= floor:
                            if score > floor:
                                score -= mismatch_pts
                            if score < floor:
                                score = floor
                        mm5 += 1
                    else:
                        score += match_pts
                    fl += 1
                    if score >= hi_score and (mm5 * 100) // (fl + core_len) <= 15:
                        hi_score, hi_len, hi_mm = score, fl, mm5
                        floor = hi_score - 4 * match_pts
                flank5, mm5 = hi_len, hi_mm
                # 3' extension (:6675-6713)
                mm3 = 0
                score = core_len * match_pts
                floor = score - 4 * match_pts
                hi_score, hi_len, hi_mm = score, 0, 0
                fl = 0
                qi, ti = this_ofs + core_len, loci + core_len
                while qi < probe_len and ti < seq_len:
                    tb = seq[left + core_len + fl] & 0x07
                    pb = probe[qi] & 0x07
                    if tb > 4 or pb > 4:
                        break
                    if tb == 4 or pb == 4 or pb != tb:
                        if score > floor:
                            score -= mismatch_pts
                        if score < floor:
                            score = floor
                        mm3 += 1
                    else:
                        score += match_pts
                    fl += 1
                    if score >= hi_score and (mm3 * 100) // (fl + core_len) <= 15:
                        hi_score, hi_len, hi_mm = score, fl, mm3
                        floor = hi_score - 4 * match_pts
                    qi += 1
                    ti += 1
                flank3, mm3 = hi_len, hi_mm
                cur = dict(id=num, qs=this_ofs - flank5, tl=loci - flank5, al=flank5 + core_len + flank3, mm=mm5 + mm3, fs=fs, tid=targ_id,
                           red=False, nxt=0)
                # redundancy (:6734-6775)
                si = targ_hash[hidx]
                while si != 0:
                    pv = hits[si - 1]
                    if not pv["red"] and pv["fs"] == cur["fs"] and pv["tid"] == cur["tid"]:
                        if not ((cur["qs"] + cur["al"] + core_len - 1) < pv["qs"] or cur["qs"] > (pv["qs"] + pv["al"] + core_len - 1)):
                            if cur["al"] + core_len // 2 <= pv["al"]:
                                cur["red"] = True
                            elif cur["al"] >= pv["al"] + core_len // 2:
                                pv["red"] = True
                            if not ((cur["tl"] + cur["al"] + core_len - 1) < pv["tl"] or cur["tl"] > (pv["tl"] + pv["al"] + core_len - 1)):
                                if cur["al"] < pv["al"]:
                                    cur["red"] = True
                                elif cur["al"] > pv["al"]:
                                    pv["red"] = True
                                elif cur["mm"] >= pv["mm"]:
                                    cur["red"] = True
                                else:
                                    pv["red"] = True
                    si = pv["nxt"]
                if cur["red"]:
                    continue
                if num < len(hits):
                    hits[num] = cur
                else:
                    hits.append(cur)
                num += 1
                cur["nxt"] = targ_hash[hidx]
                targ_hash[hidx] = num
                if num >= max_hits:
                    break
            if num >= max_hits:
                stop = True
                break
    return [(h["qs"], h["al"], h["tid"], h["tl"], h["mm"], h["id"], h["fs"]) for h in hits[:num] if not h["red"]]


def index_from_oracle(oracle, h):
    """(seq, sa, entries) of an index the CPU oracle holds (tests/oracle_bindings.py)"""
    ents = sorted(oracle.entries(h), key=lambda e: e["start_ofs"])
    return np.array(oracle.seq(h)).tobytes(), oracle.sa(h).tolist(), [(e["entry_id"], e["start_ofs"], e["seq_len"]) for e in ents]


def as_array(nodes, dtype):
    a = np.zeros(len(nodes), dtype=dtype)
    for k, f in enumerate(NODE_FIELDS):
        a[f] = [n[k] for n in nodes]
    return a
