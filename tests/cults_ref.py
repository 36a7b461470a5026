"""Sequential Python restatement of CSfxArray::GenKMerCultThreadRange, GenKMerCultsCnts (MaxHomozygotic 0) and
AntisenseKMerCultsCnts (libkit4b/SfxArray.cpp:2733-3133), loop by loop, over an index (seq bytes, suffix array list,
[(entry_id, start_ofs, seq_len)]) as tests/query_ref.py makes it; and RefIndex, which answers kit4b_amd.kmermarkers_fasta's
questions from the restatement, so that the package's host-side post-processing can be compared with the front end's files
without a device.  test_cults_cpu.py pins the restatement to the reference's recorded callbacks."""
import bisect

import numpy as np

MAX_CULTIVARS, MIN_PRE, MAX_PRE, MAX_TOT = 20000, 5, 200, 300  # SfxArray.h:186-189
UNSUPPORTED = -3

_occ_cache = {}
_low_cache = {}


def _low(index):
    """the concatenation's low nibbles as bytes (every comparison of the reference is `& 0x0f`), made once per index"""
    key = id(index[0])
    if key not in _low_cache:
        _low_cache[key] = (index[0], (np.frombuffer(index[0], dtype=np.uint8) & 0x0F).tobytes())
    return _low_cache[key][1]


def _occurrences(index, plen):
    """every exact P-mer of the concatenation -> its loci (what IterateExacts walks; the order does not matter to a count)"""
    key = (id(index[0]), plen)
    if key not in _occ_cache:
        seq = np.frombuffer(index[0], dtype=np.uint8) & 0x0F
        d = {}
        raw = seq.tobytes()
        for psn in range(len(raw) - plen + 1):
            d.setdefault(raw[psn:psn + plen], []).append(psn)
        _occ_cache[key] = (index[0], d)  # (the bytes object is kept so that its id stays taken)
    return _occ_cache[key][1]


_starts_cache = {}


def _entry_idx(entries, psn):
    """MapChunkHit2Entry: place in the entry table"""
    if id(entries) not in _starts_cache:
        _starts_cache[id(entries)] = (entries, [e[1] for e in entries])
    i = bisect.bisect_right(_starts_cache[id(entries)][1], psn) - 1
    return i if i >= 0 and psn < entries[i][1] + entries[i][2] else None


def thread_range(index, kmer_len, thread_inst, num_threads, start):
    """GenKMerCultThreadRange (:2733-2801): (rc, end)"""
    seq, sa, _ = index
    n = len(seq)
    if num_threads < 1 or num_threads > 64 or thread_inst < 1 or thread_inst > num_threads or start < 0:
        return -1, 0
    if start >= n:
        return -1, 0
    if n - start < 50000:
        return 1, n - 1
    end = start + (n - start) // (1 + num_threads - thread_inst)
    if end + 25000 >= n:
        return 1, n - 1
    psn1 = sa[end]
    end += 1
    while end < n:
        psn2 = sa[end]
        if psn2 + kmer_len >= n:
            return 1, end
        for ofs in range(kmer_len):
            a, b = seq[psn1 + ofs] & 0x0F, seq[psn2 + ofs] & 0x0F
            if a > 3 or a != b:
                return 1, end
        end += 1
    return 0, 0


def _antisense(index, plen, slen, rec):
    """AntisenseKMerCultsCnts (:3081-3133)"""
    seq, _, entries = index
    pre = bytes(3 - (b & 0x0F) for b in reversed(rec["seq"][:plen]))
    for psn in _occurrences(index, plen).get(pre, ()):
        if slen > 0 and any(psn + plen + o >= len(seq) or (seq[psn + plen + o] & 0x0F) > 3 for o in range(slen)):
            continue
        c = rec["cnts"].setdefault(_entry_idx(entries, psn), [0, 0])
        c[1] += 1
        rec["anti"] += 1


def gen_kmer_cults_cnts(index, sense_only, start, end, plen, slen, min_cult, max_homo=0, callback=None):
    """GenKMerCultsCnts (:2804-3079).  Returns (rc, records): rc the located K-mers, -1 on a parameter error, the callback's value
    when it is below 0; a record per callback: head (suffix index of the first element), seq (K index bytes), sense, anti,
    cult = [(entry_id, sense, antisense)] of the entries with a count, by place in the table."""
    seq, sa, entries = index
    n, ne, klen = len(seq), len(entries), plen + slen
    if plen < MIN_PRE or slen < 0 or plen > MAX_PRE or slen > MAX_PRE or min_cult < 0 or klen > MAX_TOT or start < 0 or end < 0:
        return -1, []
    if ne > MAX_CULTIVARS or min_cult > ne:
        return -1, []
    if min_cult == 0:
        min_cult = ne
    if start > n:
        return -1, []
    if slen and max_homo:
        return UNSUPPORTED, []
    if end == 0 or end >= n:
        end = n - 1
    recs, located = [], 0
    low = _low(index)  # (slices of it stand for the reference's base-by-base loops)

    def finish(rec):
        if not sense_only:
            _antisense(index, plen, slen, rec)
        if len(rec["cnts"]) >= min_cult:
            rec["cult"] = [(entries[i][0], c[0], c[1]) for i, c in sorted(rec["cnts"].items())]
            recs.append(rec)
            if callback is not None:
                return callback(rec)
        return 0

    cur = None
    while True:
        cur = None
        while start <= end:
            psn = sa[start]
            if psn + klen >= n:
                start += 1
                continue
            if max(low[psn:psn + klen]) <= 3:
                break
            start += 1
        if start > end:
            break
        cur = dict(head=start, seq=bytes(seq[psn:psn + klen]), low_prefix=low[psn:psn + plen], sense=1, anti=0, cnts={_entry_idx(entries, psn): [1, 0]})
        at_end = start == end
        start += 1
        if at_end:
            break
        while start <= end:
            psn2 = sa[start]
            if psn2 + klen >= n:
                break
            if low[psn2:psn2 + plen] != cur["low_prefix"]:
                break
            if slen and max(low[psn2 + plen:psn2 + klen]) > 3:
                start += 1
                continue
            cur["cnts"].setdefault(_entry_idx(entries, psn2), [0, 0])[0] += 1
            cur["sense"] += 1
            start += 1
        located += 1
        rc = finish(cur)
        if rc < 0:
            return rc, recs
        cur = None
        if not start <= end:
            break
    if cur is not None:
        located += 1
        rc = finish(cur)
        if rc < 0:
            return rc, recs
    return located, recs


def flags(index, plen, slen, start, end):
    """the parallel form's per-element X, F and b over start .. end (inclusive): what each crafted case is checked to exercise"""
    seq, sa, _ = index
    n, klen = len(seq), plen + slen
    out = []
    for i in range(start, end + 1):
        psn = sa[i]
        x = psn + klen >= n
        f = not x and all((seq[psn + o] & 0x0F) <= 3 for o in range(klen))
        b = i == start or x or any((seq[psn + o] & 0x0F if psn + o < n else 0x10) != (seq[sa[i - 1] + o] & 0x0F if sa[i - 1] + o < n else 0x20)
                                   for o in range(plen))
        out.append((x, f, b))
    return out


class RefIndex:
    """the three methods kit4b_amd.kmermarkers_fasta asks of an index, answered by the restatement"""

    def __init__(self, index):
        self.index = index

    def info(self):
        return dict(n_entries=len(self.index[2]), concat_len=len(self.index[0]))

    def kmer_cult_thread_range(self, kmer_len, thread_inst, num_threads, start):
        return thread_range(self.index, kmer_len, thread_inst, num_threads, start)

    def kmer_cults(self, prefix_len, suffix_len=0, min_cultivars=0, sense_only=False, start_sfx_idx=0, end_sfx_idx=0, **_):
        import kit4b_amd

        rc, recs = gen_kmer_cults_cnts(self.index, sense_only, start_sfx_idx, end_sfx_idx, prefix_len, suffix_len, min_cultivars)
        assert rc >= 0
        return as_arrays(kit4b_amd, rc, recs, prefix_len + suffix_len)


def as_arrays(k4, rc, recs, klen):
    """the records in the form SfxIndex.kmer_cults returns"""
    kmers = np.zeros(len(recs), dtype=k4.CULT_KMER_DTYPE)
    bases = np.zeros((len(recs), klen), dtype=np.uint8)
    dist = []
    for i, r in enumerate(recs):
        kmers[i] = (r["head"], len(dist), min(r["sense"], 0xFFFFFFFF), min(r["anti"], 0xFFFFFFFF), len(r["cult"]), 0)
        bases[i] = np.frombuffer(r["seq"], dtype=np.uint8) & 0x0F
        dist += r["cult"]
    return dict(n_located=rc, kmers=kmers, bases=bases, dist=np.array(dist, dtype=k4.CULT_DIST_DTYPE).reshape(-1))
