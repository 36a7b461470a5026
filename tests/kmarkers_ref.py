"""Sequential Python restatement, loop by loop, of CSfxArray::IterateExacts over LocateFirstExact (libkit4b/SfxArray.cpp:3381-3458,
:7938-8060), both CSfxArray::MatchesOtherChroms (:5094-5235), SetBaseFlags (:2264-2361) and CLocKMers::LocateSpeciesUniqueKMers for ONE
thread (ngskit4b/LocKMers.cpp:1085-1240), over an index (seq bytes, suffix array list, [(entry_id, start_ofs, seq_len)]) as
tests/query_ref.py makes it.  The flags are real: a bytearray beside the sequence, written in the reference's order.  It gives one
status per start locus of the targets (the numbering of include/k4sfx.h) and the marker records; RefIndex answers
kit4b_amd.kmarkers_fasta's questions from it, so the package's host side can be compared with the front end's files without a
device.  test_kmarkers_cpu.py pins all of it to the reference's recordings."""
import numpy as np

EOS = 7
NOT_KMER, FIRST_FOREIGN, DUPLICATE, FOREIGN_HIT, HAMMING, PREFIX, ACCEPTED = 1, 2, 3, 4, 5, 6, 7
ERR_PARAMS = -100

_low_cache = {}


def _low(index):
    key = id(index[0])
    if key not in _low_cache:
        _low_cache[key] = (index[0], (np.frombuffer(index[0], dtype=np.uint8) & 0x0F).tobytes() + bytes([EOS]) * 8)
    return _low_cache[key][1]


def revcomp(seq):
    return bytes(3 - b if b <= 3 else b for b in reversed(bytes(seq)))


def cmp_probe_targ(low, probe, pos):
    """CmpProbeTarg (:2508-2525)"""
    n = len(probe)
    t = low[pos:pos + n]
    if t == probe and EOS not in t:
        return 0
    for a, b in zip(probe, t):
        if b == EOS:
            return -1
        if a != b:
            return 1 if a > b else -1
    return -1  # (the concatenation ends with an end-of-sequence symbol)


def locate_first_exact(index, probe):
    """LocateFirstExact (:7938-8060) without a core table: index + 1 of the lowest matching element, or 0"""
    low, sa = _low(index), index[1]
    lo, hi = 0, len(sa) - 1
    while True:
        psn = (lo + hi) // 2
        c = cmp_probe_targ(low, probe, sa[psn])
        if c == 0:
            if psn == 0 or lo == psn:
                return psn + 1
            while True:
                if c == 0:
                    mark = psn
                    if mark == 0:
                        return mark + 1
                    hi = psn - 1
                psn = (lo + hi) // 2
                c = cmp_probe_targ(low, probe, sa[psn])
                if c == 0:
                    continue
                lo = psn + 1
                if lo == mark:
                    return mark + 1
        if c < 0:
            hi = psn - 1
        else:
            lo = psn + 1
        if hi < lo:
            return 0


def _entry_of(index, psn):
    """MapChunkHit2Entry: (entry_id, start_ofs, seq_len)"""
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


def iterate_exacts(index, probe, prev_hit_idx):
    """IterateExacts (:3381-3458): (hit index or 0, TargEntryID, HitLoci)"""
    probe = bytes(b & 0x0F for b in probe)
    low, sa = _low(index), index[1]
    if prev_hit_idx >= len(sa):
        return 0, 0, 0
    if not prev_hit_idx:
        psn = locate_first_exact(index, probe)
        if psn == 0:
            return 0, 0, 0
        psn -= 1
    else:
        if cmp_probe_targ(low, probe, sa[prev_hit_idx]) != 0:
            return 0, 0, 0
        psn = prev_hit_idx
    e = _entry_of(index, sa[psn])
    return psn + 1, e[0], sa[psn] - e[1]


def walk_exacts(index, probe):
    """IterateExacts to exhaustion: [(hit index, entry id, loci)]"""
    out, prev = [], 0
    while True:
        nxt, eid, loci = iterate_exacts(index, probe, prev)
        if nxt <= 0:
            return out
        out.append((nxt, eid, loci))
        prev = nxt


def matches_other_chroms(index, probe_ids, max_tot_mm, probe):
    """MatchesOtherChroms (:5161-5235; the single-id overload, :5094-5158, is the same with a list of one)"""
    probe = bytes(b & 0x0F for b in probe)
    low = _low(index)
    by_id = {e[0]: e for e in index[2]}
    n = len(probe)
    core_len = n // (1 + max_tot_mm)
    if core_len < 8:
        core_len = 8
    ofs = 0
    while ofs < n - core_len:
        if ofs + core_len > n:
            ofs = n - core_len
        core = probe[ofs:ofs + core_len]
        prev = 0
        while True:
            nxt, eid, loci = iterate_exacts(index, core, prev)
            if nxt <= 0:
                break
            prev = nxt
            if eid in probe_ids:
                continue
            if loci < ofs:
                continue
            e = by_id[eid]
            if ((loci + n - ofs) & 0xFFFFFFFF) > e[2]:
                continue
            targ = e[1] + loci - ofs
            num_mm, idx = 0, 0
            while num_mm > max_tot_mm and idx < n:  # (as written: never entered)
                if low[targ + idx] != probe[idx]:
                    num_mm += 1
                idx += 1
            if num_mm <= max_tot_mm:
                return 1
        ofs += core_len
    return 0


def check_params(index, target_ids, kmer_len, min_hamming, mode, prefix_len):
    ids = [e[0] for e in index[2]]
    if not 20 <= kmer_len <= 100 or not 1 <= min_hamming <= 5 or mode not in (0, 1, 2):
        return ERR_PARAMS
    if mode == 2 and not 10 <= prefix_len <= kmer_len - 10:
        return ERR_PARAMS
    if not 1 <= len(target_ids) <= 50 or len(set(target_ids)) != len(target_ids) or any(t not in ids for t in target_ids):
        return ERR_PARAMS
    if len(target_ids) >= len(ids):
        return ERR_PARAMS
    return 0


def species_kmers(index, target_ids, kmer_len, min_hamming=1, mode=0, prefix_len=0, min_with_prefix=0):
    """LocateSpeciesUniqueKMers by one thread over the targets in the order given (the front end's: by name).  Returns
    (status bytes in target-list order, [processed, cultivar specific, Hamming retained, accepted], [marker sequences])."""
    low = _low(index)
    by_id = {e[0]: e for e in index[2]}
    flags = bytearray(len(index[0]))  # the high nibbles of the sequence bytes
    targets = set(target_ids)
    others = len(index[2]) - len(target_ids)
    if mode == 2 and (min_with_prefix == 0 or min_with_prefix > others):  # :719-720
        min_with_prefix = others
    if mode != 2:
        prefix_len = 0

    def set_flags(eid, loci):
        p = by_id[eid][1] + loci
        prior = flags[p]
        flags[p] |= 0x01
        return prior

    status, tallies, markers = [], [0, 0, 0, 0], []
    for tid in target_ids:
        _, start, seq_len = by_id[tid]
        st = bytearray([NOT_KMER]) * seq_len
        seq = low[start:start + seq_len]
        end = 0
        while end < seq_len:  # the do-loop over the ACGT subsequences of a block (:1085-1091)
            s0 = end
            while end < seq_len and seq[end] <= 3:
                end += 1
            cur_len = end - s0
            end += 1
            if cur_len < kmer_len:
                continue
            mark_len, mark_start_idx, mark_start = 0, 0, 0
            for start_idx in range(cur_len - kmer_len + 1):
                loc = s0 + start_idx
                kmer = seq[loc:loc + kmer_len]
                rc = revcomp(kmer)
                tallies[0] += 1
                targ_hit = non_targ = is_dup = False
                prev, rcpl_idx = 0, 0
                first_foreign = False
                while True:
                    nxt, eid, loci = iterate_exacts(index, kmer, prev)
                    if nxt <= 0:
                        break
                    if not prev and eid in targets:
                        rcpl_idx, r_eid, r_loci = iterate_exacts(index, rc, 0)
                        if rcpl_idx != 0:
                            f = set_flags(eid, loci)
                            f |= set_flags(r_eid, r_loci) << 4  # (prior flags of the second locus in bits 4..7)
                        else:
                            f = set_flags(eid, loci)
                        if f & 0x11:
                            is_dup = True
                            break
                    if eid in targets:
                        targ_hit = True
                    else:
                        non_targ = True
                        first_foreign = not prev
                        break
                    prev = nxt
                if non_targ or is_dup:
                    st[loc] = DUPLICATE if is_dup else (FIRST_FOREIGN if first_foreign else FOREIGN_HIT)
                    continue
                prev = rcpl_idx
                while True:
                    nxt, eid, loci = iterate_exacts(index, rc, prev)
                    if nxt <= 0:
                        break
                    if eid in targets:
                        targ_hit = True
                    else:
                        non_targ = True
                        break
                    prev = nxt
                if non_targ or not targ_hit:
                    st[loc] = FOREIGN_HIT
                    continue
                tallies[1] += 1
                matches = 0
                if min_hamming > 1:
                    matches = matches_other_chroms(index, target_ids, min_hamming - 1, kmer)
                    if not matches:
                        matches = matches_other_chroms(index, target_ids, min_hamming - 1, rc)
                if matches:
                    st[loc] = HAMMING
                    continue
                tallies[2] += 1
                if mode == 2 and prefix_len:
                    seen, n_pref = set(), 0
                    for probe in (kmer[:prefix_len], rc[:prefix_len]):
                        prev = 0
                        while n_pref < min_with_prefix:
                            nxt, eid, loci = iterate_exacts(index, probe, prev)
                            if nxt <= 0:
                                break
                            prev = nxt
                            if eid in targets:
                                continue
                            if eid not in seen:
                                seen.add(eid)
                                n_pref += 1
                        if n_pref >= min_with_prefix:
                            break
                    if n_pref < min_with_prefix:
                        st[loc] = PREFIX
                        continue
                st[loc] = ACCEPTED
                if mode != 1:  # (:1209: eKMPMNoExtdKMers is the mode that extends)
                    markers.append(kmer)
                    tallies[3] += 1
                    continue
                if mark_len and start_idx > mark_start_idx + 1:
                    markers.append(seq[mark_start:mark_start + mark_len])
                    tallies[3] += 1
                    mark_len = 0
                if mark_len == 0:
                    mark_len, mark_start = kmer_len, loc
                else:
                    mark_len += 1
                mark_start_idx = start_idx
            if mode == 0 and mark_len:  # (:1233: never true, mode 0 builds no run)
                markers.append(seq[mark_start:mark_start + mark_len])
                tallies[3] += 1
        status.append(bytes(st))
    return b"".join(status), tallies, markers


def marker_file(cultivar, kmer_len, printed_hamming, markers):
    """ReportMarker (:192-223)"""
    out = []
    for i, m in enumerate(markers):
        m = m[:4000]
        out.append(">%sM%d %d|%d|%d\n%s\n" % (cultivar, i + 1, len(m), kmer_len, printed_hamming, "".join("ACGTN"[min(b, 4)] for b in m)))
    return "".join(out).encode()


class RefIndex:
    """what kit4b_amd.kmarkers_fasta asks of an index, answered by the restatement"""

    def __init__(self, index, names):
        self.index, self.names = index, names
        self.low = _low(index)

    def info(self):
        return dict(n_entries=len(self.index[2]))

    def entry(self, entry_id):
        e = [x for x in self.index[2] if x[0] == entry_id][0]
        return dict(entry_id=e[0], name=self.names[e[0] - 1], seq_len=e[2], start_ofs=e[1], end_ofs=e[1] + e[2] - 1)

    def get_seq(self, entry_id, loci, length):
        e = [x for x in self.index[2] if x[0] == entry_id][0]
        return np.frombuffer(self.low[e[1] + loci:e[1] + min(loci + length, e[2])], dtype=np.uint8)

    def species_kmers(self, target_ids, kmer_len, min_hamming=1, mode=0, prefix_len=0, min_with_prefix=0):
        st, tallies, _ = species_kmers(self.index, list(target_ids), kmer_len, min_hamming, mode, prefix_len, min_with_prefix)
        return np.frombuffer(st, dtype=np.uint8), dict(zip(("processed", "cultivar_specific", "hamming_retained", "accepted"), tallies))
