"""CSfxArray::LocateSfxHammings (libkit4b/SfxArray.cpp:4107-4220), LocateHammings (:4227-4331) and LocateHamming (:4339-4627)
restated literally and sequentially in Python (CPU).  tests/test_hamm_cpu.py pins it byte for byte to what the reference itself
returned (tests/golden/hamm_*.xz), so that the GPU tests may use it on fresh inputs where the reference is absent.

An index is (seq, sa, entries) as in query_ref.py: the concatenated sequence as bytes (codes 0..4, 7 behind every target), its
suffix array as a list, [(entry_id, start_ofs, seq_len)] sorted by start.  `stats`, when given, is a dict of counters: which stage
found the neighbour ("stage<hmin>"), "abandoned" (a run given up at the MinCoreDepth count), "capped" (a walk ended by
MaxCoreDepth), "dup_skip", "eos_break", "before_start", "past_end", "self_skip", "filter_skip".

Within a capped run the occurrences explored depend on the order of suffixes that tie through an end-of-sequence symbol, which
index builders are free to choose: `assert_no_tie` makes a capped walk fail when its run holds two suffixes that compare equal
up to an EOS.
"""
import bisect

from query_ref import _cmp, revcomp  # CmpProbeTarg (:2508-2525)

ERR_INTERNAL = -1


def _first_exact(index, core):
    """LocateFirstExact (:7938-8058): index of the first suffix that holds core, or -1"""
    seq, sa, _ = index
    lo, hi = 0, len(sa)
    while lo < hi:
        mid = (lo + hi) // 2
        if _cmp(core, seq, int(sa[mid])) > 0:
            lo = mid + 1
        else:
            hi = mid
    return lo if lo < len(sa) and _cmp(core, seq, int(sa[lo])) == 0 else -1


def _last_exact(index, core, first):
    """LocateLastExact (:8227-8351): index of the last suffix that holds core"""
    seq, sa, _ = index
    lo, hi = first, len(sa)
    while lo < hi:
        mid = (lo + hi) // 2
        if _cmp(core, seq, int(sa[mid])) >= 0:
            lo = mid + 1
        else:
            hi = mid
    return lo - 1


def _map_entry(index, ofs):
    _, _, entries = index
    k = bisect.bisect_right([e[1] for e in entries], ofs) - 1
    e = entries[k]
    assert e[1] <= ofs < e[1] + e[2]
    return e


def _iterate_exacts(index, probe):
    """IterateExacts (:3382-3458): (entry id, locus) of every exact occurrence in suffix-array order"""
    seq, sa, _ = index
    i = _first_exact(index, probe)
    while i >= 0 and i < len(sa) and _cmp(probe, seq, int(sa[i])) == 0:
        e = _map_entry(index, int(sa[i]))
        yield e[0], int(sa[i]) - e[1]
        i += 1


def _bump(stats, key):
    if stats is not None:
        stats[key] = stats.get(key, 0) + 1


def _tie_through_eos(seq, a, b, core_len):
    """do the suffixes at a and b (both hold the same core) compare equal up to an EOS?"""
    j = core_len
    while True:
        x = seq[a + j] & 0x0F if a + j < len(seq) else 7
        y = seq[b + j] & 0x0F if b + j < len(seq) else 7
        if x == 7 or y == 7:
            return x == 7 and y == 7
        if x != y:
            return False
        j += 1


def locate_hamming(index, hmin, hmax, min_cd, max_cd, both, probe, probe_entry, probe_loci, iib, stats=None, assert_no_tie=True):
    seq, sa, _ = index
    n = len(seq)
    probe = [int(b) & 0x0F for b in probe]
    plen = len(probe)
    if hmin == 0:
        for tid, loci in _iterate_exacts(index, probe):
            if probe_entry == tid and probe_loci == loci:
                _bump(stats, "self_skip")
                continue
            if probe_entry != 0 and iib != 0 and ((iib == 1 and probe_entry != tid) or (iib == 2 and probe_entry == tid)):
                _bump(stats, "filter_skip")
                continue
            return 0
        if both:
            for tid, loci in _iterate_exacts(index, [int(b) for b in revcomp(probe)]):
                if probe_entry != 0 and iib != 0 and ((iib == 1 and probe_entry != tid) or (iib == 2 and probe_entry == tid)):
                    _bump(stats, "filter_skip")
                    continue
                return 0
    if hmax == 0:
        return 1
    core_len = plen // (hmax + 1)
    cur = plen // core_len
    antisense = False
    while True:
        max_seg = plen // core_len
        for seg in range(max_seg):
            seg_ofs = seg * core_len
            core = probe[seg_ofs:seg_ofs + core_len]
            ti = _first_exact(index, core)
            if ti < 0:
                continue
            first = ti
            it = 0
            copies = 0
            while cur > hmin and it < max_cd:
                it += 1
                if it > 1:
                    if ti + 1 >= n or int(sa[ti + 1]) + core_len > n:
                        break
                    if it == min_cd and not copies:
                        last = _last_exact(index, core, first)
                        copies = 1 + (last + 1) - ti
                        if max_cd and copies > max_cd:
                            _bump(stats, "abandoned")
                            break
                    nxt = int(sa[ti + 1])
                    ok = True
                    for j in range(core_len):
                        t = seq[nxt + j] & 0x0F
                        if t == 7 or t == 4 or core[j] != t:
                            ok = False
                            break
                    if not ok:
                        break
                    ti += 1
                    if it == max_cd:
                        _bump(stats, "capped")
                        if assert_no_tie:
                            last = _last_exact(index, core, first)
                            run = [int(sa[k]) for k in range(first, last + 1)]
                            if last > ti:  # (a run explored to its end is explored whatever its order)
                                for a in range(len(run)):
                                    for b in range(a + 1, len(run)):
                                        assert not _tie_through_eos(seq, run[a], run[b], core_len), "tie through EOS inside a capped run"
                pos = int(sa[ti])
                if pos < seg_ofs:
                    _bump(stats, "before_start")
                    continue
                left = pos - seg_ofs
                if left + plen > n:
                    _bump(stats, "past_end")
                    continue
                if seg > 0:
                    dup = False
                    for d in range(seg):
                        if _cmp(probe[d * core_len:(d + 1) * core_len], seq, left + d * core_len) == 0:
                            dup = True
                            break
                    if dup:
                        _bump(stats, "dup_skip")
                        continue
                sub = 0
                j = 0
                while j < plen:
                    t = seq[left + j] & 0x0F
                    if t == 7:
                        _bump(stats, "eos_break")
                        break
                    if probe[j] == 4 or probe[j] == t:
                        j += 1
                        continue
                    sub += 1
                    if sub > cur:
                        break
                    j += 1
                if j != plen:
                    continue
                if sub == 0 and not antisense and probe_entry > 0:
                    e = _map_entry(index, left)
                    if probe_entry == e[0] and probe_loci == left - e[1]:
                        _bump(stats, "self_skip")
                        continue
                    if iib != 0 and ((iib == 1 and probe_entry != e[0]) or (iib == 2 and probe_entry == e[0])):
                        _bump(stats, "filter_skip")
                        continue
                if sub < cur:
                    cur = sub
                    if stats is not None:
                        stats["found"] = (hmin, seg, "-" if antisense else "+", sub)
            if cur <= hmin:
                break
        if cur > hmin and both:
            probe = [int(b) for b in revcomp(probe)]
            both = False
            probe_entry = 0
            antisense = True
        else:
            antisense = False
        if not (cur > hmin and antisense):
            break
    return cur


def _escalate(index, rhamm, both, min_cd, max_cd, probe, entry, loci, iib, stats, assert_no_tie):
    def lh(hmin, hmax, mn, mx):
        r = locate_hamming(index, hmin, hmax, mn & 0xFFFFFFFF, mx & 0xFFFFFFFF, both, probe, entry, loci, iib, stats, assert_no_tie)
        if stats is not None:
            stats["last_stage"] = hmin
        return r

    r = lh(0, 1, 2 * min_cd, 10 * max_cd)
    if r > 1 and rhamm > 1:
        r = lh(2, 2, 2 * min_cd, 8 * max_cd)
        if r > 2 and rhamm > 2:
            r = lh(3, 3, 2 * min_cd, 4 * max_cd)
            if r > 3 and rhamm > 3:
                r = lh(4, 4, min_cd, 2 * max_cd)
                if r > 4 and rhamm > 4:
                    r = lh(5, rhamm, min_cd, max_cd)
    return r


def _kmers(index, rhamm, both, kmer_len, nth, src, min_cd, max_cd, entry, loci0, iib, out, out_ofs, clamp, stats, assert_no_tie):
    if nth <= 0:
        nth = 1
    for ofs in range(0, len(src) - kmer_len + 1, nth):
        kmer = [int(b) & 0x0F for b in src[ofs:ofs + kmer_len]]
        n_idx = []
        for i, b in enumerate(kmer):
            if b >= 4:
                n_idx.append(i)
                if len(n_idx) > 4:
                    break
        if len(n_idx) > 4:
            out[out_ofs + ofs] = 0
            continue
        lowest = 0x7F
        it = 0
        while True:
            if n_idx:
                for k, i in enumerate(n_idx):
                    kmer[i] = (it >> (2 * k)) & 3
                it += 1
            st = None if stats is None else {}
            r = _escalate(index, rhamm, both, min_cd, max_cd, kmer, entry, loci0 + ofs, iib, st, assert_no_tie)
            if stats is not None:
                stats.setdefault("kmers", {}).setdefault(out_ofs + ofs, []).append(st)
            if (r & 0x7F) < lowest:
                lowest = r & 0x7F
            if lowest == 0 or not n_idx or it >= 4 ** len(n_idx):
                break
        if clamp and lowest > 20:
            lowest = 20
        out[out_ofs + ofs] = lowest


def locate_sfx_hammings(index, rhamm, both, kmer_len, nth, span_len, min_cd, max_cd, entry_id, entry_loci, iib, out, out_ofs=0, stats=None,
                        assert_no_tie=True):
    """writes out[out_ofs + j] for the sampled j; returns 0 or the reference's error code"""
    seq, _, entries = index
    if entry_id == 0 or rhamm < 1 or kmer_len < 10 or kmer_len > 500 or span_len < kmer_len:
        return ERR_INTERNAL
    ent = [e for e in entries if e[0] == entry_id]
    if not ent or ent[0][2] == 0 or entry_loci > ent[0][2] or ent[0][2] - entry_loci < span_len:
        return ERR_INTERNAL
    start = ent[0][1] + entry_loci
    _kmers(index, rhamm, both, kmer_len, nth, seq[start:start + span_len], min_cd, max_cd, entry_id, entry_loci, iib, out, out_ofs, True, stats,
           assert_no_tie)
    return 0


def locate_hammings(index, rhamm, both, kmer_len, nth, src, min_cd, max_cd, iib, out, out_ofs=0, stats=None, assert_no_tie=True):
    """the LocateHammings form with SeqEntry 0 / SeqLoci 0"""
    if rhamm < 1 or kmer_len < 10 or kmer_len > 500 or len(src) < kmer_len:
        return ERR_INTERNAL
    _kmers(index, rhamm, both, kmer_len, nth, src, min_cd, max_cd, 0, 0, iib, out, out_ofs, False, stats, assert_no_tie)
    return 0
