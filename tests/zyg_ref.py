"""Sequential Python restatement of CSfxArray::LocateAllNearMatches (libkit4b/SfxArray.cpp:4820-5091) and of `genzygosity`'s scan
(genzygosity/genzygosity.cpp:1122-1236 as one thread runs it, the parameter derivation of :681-697 and :998-1027, the two result
files of :746-771) over an index (seq bytes, suffix array list, [(entry_id, start_ofs, seq_len)]) as tests/query_ref.py makes it.
The core loop, the walk with its three skips and four stops, the ident-node limit and MaxMatches are carried literally; the hash of
tsIdentNode is a set with a count.  LocateFirstExact / LocateLastExact are answered from a table of the runs of every core length
asked for (a run is one stretch of the array, which the recordings of tests/golden/kmarkers_calls.xz show).  RefIndex answers
kit4b_amd.genzygosity_csv's questions from the restatement.  test_zygosity_cpu.py pins all of it to the reference's recordings."""
import numpy as np

EOS = 7
N_ = 4
ERR_PARAMS = -100
NODES = 1024000  # cMaxNumIdentNodes per thread
PASSED_OVER, NOT_UNIQUE, UNIQUE, UNIQUE_MATCHED = 0, 1, 2, 3
TOTALS = ("windows", "passed_over", "rejected", "unique", "unique_matched", "ordered", "second_launch")

_cache = {}


def _low(index):
    key = ("low", id(index[0]))
    if key not in _cache:
        low = (np.frombuffer(index[0], dtype=np.uint8) & 0x0F).tobytes() + bytes([EOS]) * 8
        _cache[key] = (index[0], low, np.frombuffer(low, dtype=np.uint8))
    return _cache[key][1], _cache[key][2]


def _runs(index, core_len):
    """{core bytes: (first index, count)} over the suffix array"""
    key = ("runs", id(index[0]), core_len)
    if key not in _cache:
        low, _ = _low(index)
        runs, prev = {}, None
        for i, p in enumerate(index[1]):
            c = low[p:p + core_len]
            if EOS in c or len(c) < core_len:
                prev = None
                continue
            if c == prev:
                runs[c][1] += 1
            else:
                assert c not in runs
                runs[c] = [i, 1]
                prev = c
        _cache[key] = (index[0], runs)
    return _cache[key][1]


def revcomp(seq):
    return bytes(3 - b if b <= 3 else b for b in reversed(bytes(seq)))


def core_offsets(probe_len, core_len, core_delta, max_slides):
    """the offsets the loop of :4906-4917 visits while the node limit does not end it"""
    out, ofs, delta, slides = [], 0, core_delta, 0
    while slides < max_slides and ofs <= probe_len - core_len and delta > core_len // 3:
        if ofs + core_len + delta > probe_len:
            delta = probe_len - (ofs + core_len)
        out.append(ofs)
        slides += 1
        ofs += delta
    return out


def _entry_of(index, psn):
    ents = index[2]
    lo, hi = 0, len(ents) - 1
    while hi >= lo:
        mid = (lo + hi) // 2
        if ents[mid][1] > psn:
            hi = mid - 1
        elif ents[mid][1] + ents[mid][2] - 1 >= psn:
            return ents[mid]
        else:
            lo = mid + 1
    return None


def needs_ordered_walk(index, probe, core_len, core_delta, max_slides, cur_max_iter, n_ident_nodes):
    """a pass holds a run longer than CurMaxIter, or its runs together reach the node limit"""
    p = bytes(b & 0x0F for b in probe)
    runs = _runs(index, core_len)
    for s in (p, revcomp(p)):
        cnts = [runs.get(s[o:o + core_len], (0, 0))[1] for o in core_offsets(len(p), core_len, core_delta, max_slides)]
        if (cur_max_iter and any(c > cur_max_iter for c in cnts)) or sum(cnts) >= n_ident_nodes:
            return True
    return False


def near_matches(index, max_tot_mm, core_len, core_delta, max_slides, max_matches, num_entries, probe_entry, probe_ofs, probe,
                 cur_max_iter=0, n_ident_nodes=NODES, stats=None):
    """LocateAllNearMatches: (return value, pEntryMatches as a list of num_entries counts).  stats (a dict) counts the walks that
    were cut: 'truncated' by CurMaxIter or by the check at the 100th iteration, 'node_cut' by the ident-node limit; and the reason
    of a -1: 'own_entry' or 'too_many'."""
    low, low_np = _low(index)
    sa = index[1]
    n = len(sa)
    runs = _runs(index, core_len)
    counts = [0] * max(num_entries, 0)
    plen = len(probe)
    p = bytes(b & 0x0F for b in probe)
    total = 0
    for strand in (0, 1):
        if strand:
            p = revcomp(p)
        p_np = np.frombuffer(p, dtype=np.uint8)
        delta, slides, ofs = core_delta, 0, 0
        seen, nodes = set(), 0
        while slides < max_slides and ofs <= plen - core_len and delta > core_len // 3 and nodes < n_ident_nodes:
            if ofs + core_len + delta > plen:
                delta = plen - (ofs + core_len)
            first, cnt = runs.get(p[ofs:ofs + core_len], (0, 0))
            idx, iter_cnt, num_copies, first_iter = first, 0, 0, True
            while cnt and (not cur_max_iter or iter_cnt < cur_max_iter):
                if nodes >= n_ident_nodes:
                    if stats is not None:
                        stats["node_cut"] = stats.get("node_cut", 0) + 1
                    break
                if not first_iter:
                    if idx + 1 >= first + cnt:  # the next suffix no longer matches the core, or the array ends
                        break
                    if iter_cnt == 100 and not num_copies:
                        num_copies = 1 + (first + cnt) - idx  # LocateLastExact gives index + 1 of the run's last element
                        if cur_max_iter and num_copies > cur_max_iter:
                            if stats is not None:
                                stats["truncated"] = stats.get("truncated", 0) + 1
                            break
                    idx += 1
                first_iter = False
                loc = sa[idx]
                if loc < ofs:
                    continue
                left = loc - ofs
                if left + plen > n:
                    continue
                tid = (1 + loc - ofs) & 0xFFFFFFFF
                if tid in seen:
                    continue
                seen.add(tid)
                nodes += 1
                iter_cnt += 1
                t = low[left:left + plen]
                if EOS in t or (t != p and int(np.count_nonzero(low_np[left:left + plen] != p_np)) > max_tot_mm):
                    continue
                e = _entry_of(index, left)
                if probe_entry == e[0]:
                    if probe_ofs == left - e[1]:
                        continue
                    if stats is not None:
                        stats["own_entry"] = stats.get("own_entry", 0) + 1
                    return -1, counts
                if max_matches > 0 and total == max_matches:
                    if stats is not None:
                        stats["too_many"] = stats.get("too_many", 0) + 1
                    return -1, counts
                if e[0] <= num_entries:
                    counts[e[0] - 1] += 1
                total += 1
            else:
                if cnt and stats is not None and idx + 1 < first + cnt:
                    stats["truncated"] = stats.get("truncated", 0) + 1
            slides += 1
            ofs += delta
    return total, counts


def derive(tot_seqs_len, subseq_len, max_subs, mode):
    """(CoreLen, MaxNumSlides, MaxIter) as the front end derives them"""
    min_core = 5 if tot_seqs_len < 20000000 else 8 if tot_seqs_len < 250000000 else 10
    min_core += (4, 2, 0, 6)[mode]
    return max(min_core, subseq_len // (max_subs + 1)), (4, 6, 8, 3)[mode], (5000, 25000, 50000, 1000)[mode]


def check_params(index, subseq_len=25, max_subs=2, max_ns=1, max_matches=5000, mode=0, src_first=1, src_count=None):
    n = len(index[2])
    if not 20 <= subseq_len <= 1000 or not 0 <= max_subs <= min(30, subseq_len - 18) or not 0 <= max_ns <= 5:
        return ERR_PARAMS
    if not 0 <= max_matches <= 1000000 or not 0 <= mode <= 3 or not 1 <= src_first <= n:
        return ERR_PARAMS
    if src_count is not None and (src_count < 0 or src_first + src_count - 1 > n):
        return ERR_PARAMS
    return 0


def zygosity(index, subseq_len=25, max_subs=2, max_ns=1, max_matches=5000, mode=0, src_first=1, src_count=None):
    """the scan over the source entries src_first .. src_first + src_count - 1 (ordinals of the entry table, which are the ids of an
    index the reference built): (matrix src_count x n_entries, subseqs, totals dict, status bytes of every start locus of those
    entries).  An entry shorter than subseq_len has no windows; totals['ordered'] counts the windows needs_ordered_walk names."""
    seq, sa, ents = index
    low, _ = _low(index)
    n_ent = len(ents)
    if src_count is None:
        src_count = n_ent - src_first + 1
    core_len, slides, max_iter = derive(sum(e[2] for e in ents), subseq_len, max_subs, mode)
    matrix = np.zeros((src_count, n_ent), dtype=np.uint32)
    subseqs = np.zeros(src_count, dtype=np.uint32)
    tot = dict.fromkeys(TOTALS, 0)
    status = bytearray()
    for r in range(src_count):
        eid, start, ln = ents[src_first - 1 + r]
        st = bytearray(ln)
        for loci in range(0, ln - subseq_len + 1):
            tot["windows"] += 1
            w = bytes(b & 0x07 for b in low[start + loci:start + loci + subseq_len])
            if max(w) > N_ or w.count(N_) > max_ns:
                tot["passed_over"] += 1
                continue
            tot["ordered"] += needs_ordered_walk(index, w, core_len, core_len, slides, max_iter, NODES)
            rslt, counts = near_matches(index, max_subs, core_len, core_len, slides, max_matches, n_ent, eid, loci, w, max_iter, NODES)
            if rslt < 0:
                st[loci] = NOT_UNIQUE
                tot["rejected"] += 1
                continue
            subseqs[r] += 1
            tot["unique"] += 1
            st[loci] = UNIQUE_MATCHED if rslt > 0 else UNIQUE
            if rslt > 0:
                tot["unique_matched"] += 1
                matrix[r] += np.array(counts, dtype=np.uint32) > 0
        status += st
    return matrix, subseqs, tot, np.frombuffer(bytes(status), dtype=np.uint8)


class RefIndex:
    """what kit4b_amd.genzygosity_csv asks of an index, answered by the restatement"""

    def __init__(self, index, names):
        self.index, self.names = index, names
        self.n_entries = len(names)

    def entry(self, entry_id):
        return {"name": self.names[entry_id - 1], "seq_len": self.index[2][entry_id - 1][2]}

    def zygosity(self, **kw):
        m, s, t, _ = zygosity(self.index, **kw)
        return m, s, t
