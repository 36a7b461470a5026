"""Batches larger than one grid of the step kernels (kit4b_amd/csrc/k4_align.hip), checked read for read at the cost of a few
thousand oracle reads: a read's result does not depend on its neighbours in the batch, so a small pool goes through the CPU
oracle once and the batch names every pool read many times (tile / expect / same).

slot_model restates, in plain Python, how k4k_align_step and launch_steps hand out the slots of the survivor list and of the
deferred list of a split first launch.  It needs no GPU and no library; tests/test_bigbatch_cpu.py holds it against the size of
the buffers (k4_survivor_slots), and no GPU test sends a shape it puts outside them (fits)."""
import math

import numpy as np

G = 524288        # lanes of one full grid, in every length class: launch_steps' full = 256 * 8 * (256 / K4_BS) blocks of K4_BS lanes
K4_CHUNK = 512    # k4_align_common.h: survivor slots a wave reserves per atomic
K4_SLOW_WAVES = 8192
K4_HUGE_WAVES = 256
K4_DEEP_BUCKET = 24
K4_DEFER_MIN_FRAC = 0.002
SHARES = (0, 0.05, 0.5, 0.85, 0.95, 1)


# ---- a pool tiled to a batch ---------------------------------------------------------------------------------------------------
def tile(pool_reads, m, seed, tail=0):
    """((cat, offs, lens), pool_idx): the batch that names every pool read m times and the first `tail` pool reads once more, in
    a seeded random order.  cat holds each pool read once -- kit4b_amd._flatten takes the tuple as it is and the host entry
    uploads max(offs + lens) bytes, so repeated offsets are legal."""
    assert 0 < len(pool_reads) <= 4096 and 0 <= tail <= len(pool_reads)
    p_lens = np.array([len(r) for r in pool_reads], dtype=np.uint32)
    p_offs = np.zeros(len(pool_reads), dtype=np.uint64)
    p_offs[1:] = np.cumsum(p_lens[:-1], dtype=np.uint64)
    cat = np.ascontiguousarray(np.concatenate(pool_reads), dtype=np.uint8)
    pool_idx = np.concatenate([np.tile(np.arange(len(pool_reads), dtype=np.int64), m), np.arange(tail, dtype=np.int64)])
    np.random.default_rng(seed).shuffle(pool_idx)
    return (cat, np.ascontiguousarray(p_offs[pool_idx]), np.ascontiguousarray(p_lens[pool_idx])), pool_idx


def expect(oracle_result, pool_idx):
    """the oracle's per-pool arrays in batch order (its counters, which are sums, stay behind)"""
    return {k: v[pool_idx] for k, v in oracle_result.items() if isinstance(v, np.ndarray)}


def _live_slots(want, max_hits):
    """hit slots the call fills per read, as same_kalign / same_raw (tests/test_gpu_step_plan.py) compute nh"""
    rslt, inst = (want["out"]["hit_rslt"], want["out"]["inst"]) if "out" in want else (want["rslt"], want["inst"])
    return np.where(np.isin(rslt, (1, 2, 3)), np.clip(inst, 0, max_hits), 0)


def mismatches(got, want, max_hits):
    """{what: batch indices} of everything that differs: the records (kalign form: `out`, every field; raw form: rslt, inst, low,
    nxt), the hit slots in front of nh and, in the raw form, hit slots behind nh that are not zero"""
    bad = {}
    for k in (("out",) if "out" in want else ("rslt", "inst", "low", "nxt")):
        b = np.nonzero(got[k] != want[k])[0]
        if len(b):
            bad[k] = b
    n, mh = want["hits"].shape
    assert got["hits"].shape == (n, mh) and mh == max(1, max_hits)
    gv = np.ascontiguousarray(got["hits"]).view(np.uint64).reshape(n, mh, 2)  # a k4_hit is 16 bytes
    wv = np.ascontiguousarray(want["hits"]).view(np.uint64).reshape(n, mh, 2)
    live = np.arange(mh)[None, :] < _live_slots(want, max_hits)[:, None]
    b = np.nonzero(((gv != wv).any(axis=2) & live).any(axis=1))[0]
    if len(b):
        bad["hits"] = b
    if "out" not in want:
        b = np.nonzero(((gv != 0).any(axis=2) & ~live).any(axis=1))[0]
        if len(b):
            bad["stale hit slots"] = b
    return bad


def same(got, want, max_hits, what, pool_idx=None):
    """got == want over whole arrays; on a mismatch the first eight batch indices, their pool indices and both records"""
    for k, b in mismatches(got, want, max_hits).items():
        b = b[:8]
        f = "hits" if k in ("hits", "stale hit slots") else k
        raise AssertionError((what, k, "batch", b.tolist(), "pool", None if pool_idx is None else pool_idx[b].tolist(),
                              "got", got[f][b].tolist(), "want", want[f][b].tolist()))


# ---- the chunk arithmetic of the step kernels ----------------------------------------------------------------------------------
def survivor_slots(cap):
    """k4_survivor_slots (kit4b_amd/csrc/k4_align.hip): slots of one survivor buffer, ids[b] / rows[b], for batches of up to cap reads"""
    return cap + cap // 7 + 2 * 2048 * 4 * K4_CHUNK + K4_CHUNK


def reserved_slots(n):
    """what k4_reserve sets aside for a batch of n reads on a fresh handle: cap is n rounded up to 256"""
    return survivor_slots((n + 255) // 256 * 256)


def _rate(v):
    """survivors (or reads set aside) among r real entries of a 64-slot segment: a callable, or a number per 64, rounded up"""
    return v if callable(v) else (lambda r: min(r, int(math.ceil(r * v / 64 - 1e-9))))


def _wave_pass(reals, place, defer=None):
    """one wave of one launch over its 64-slot segments (reals[p] real entries in pass p): the chunks it takes from out_count and,
    with `defer`, from ctl[K4_CTL_DEFER], each as [pass of the atomic, entries placed].  cnt > ch_left retires the tail."""
    out, dfr = [], []
    ch_left = dch_left = 0
    for p, r in enumerate(reals):
        d = defer(r) if defer else 0
        if d:
            if d > dch_left:
                dfr.append([p, 0])
                dch_left = K4_CHUNK
            dfr[-1][1] += d
            dch_left -= d
        cnt = place(r - d)
        if cnt:
            if cnt > ch_left:
                out.append([p, 0])
                ch_left = K4_CHUNK
            out[-1][1] += cnt
            ch_left -= cnt
    return out, dfr


def _worst_chunks(real, waves, passes):
    """most chunks that `real` placed entries can take when they fall on the waves and passes in the worst way: every wave that
    places anything ends in a partly used chunk, and a wave moves on from a chunk no earlier than at K4_CHUNK - 63 entries (a ballot
    holds at most 64, so the retired tail is at most 63 slots); one atomic per wave and pass at the most"""
    if real <= 0:
        return 0
    w = min(waves, real)
    return min(waves * passes, w + (real - w) // (K4_CHUNK - 63))


def slot_model(n, nch, per_wave_survivors, per_wave_deferred=None, placement="even"):
    """Slots that step 0 of a batch of n reads takes from out_count (the survivor list, ids[0] / rows[0]) and from
    ctl[K4_CTL_DEFER] (the deferred list, ids[1]).  per_wave_survivors / per_wave_deferred: of 64 real entries a wave meets in one
    pass of its stride loop, how many survive / are set aside by the first launch (a number, or a callable of the real entries of
    the segment); per_wave_deferred None is the launch that is not split.  With it the model runs both launches, the second
    walking the deferred list the first wrote, holes included, and appending to the same survivor list.

    placement "even": every segment places its share; chunks are handed out pass by pass, waves in order.  "worst": the totals of
    the even shares, placed as _worst_chunks describes (an upper bound whatever the order of the atomics)."""
    bs = 128 if nch >= 16 else 256                     # K4_BS
    full = 256 * 8 * (256 // bs)                       # launch_steps
    blocks = min((n + bs - 1) // bs, full)             # grid0
    waves = blocks * (bs // 64)
    stride = waves * 64
    place, defer = _rate(per_wave_survivors), (None if per_wave_deferred is None else _rate(per_wave_deferred))
    res = dict(grid_blocks=blocks, waves=waves, passes=-(-n // stride), defer_slots=0, deferred=0)
    if placement == "worst":
        w1, p1 = min(waves, -(-n // 64)), res["passes"]
        d = defer(64) * (n // 64) + defer(n % 64) if defer else 0
        s1 = place(64 - (defer(64) if defer else 0)) * (n // 64) + place(n % 64 - (defer(n % 64) if defer else 0))
        chunks, s2 = _worst_chunks(s1, w1, p1), 0
        if defer:
            res["defer_slots"] = K4_CHUNK * _worst_chunks(d, w1, p1)
            s2 = min(d, place(64) * -(-d // 64))
            chunks += _worst_chunks(s2, min(waves, res["defer_slots"] // 64), -(-res["defer_slots"] // stride))
        res.update(out_slots=K4_CHUNK * chunks, survivors=s1 + s2, deferred=d)
        return res
    assert placement == "even"
    memo = {}

    def run(reals, dfr):
        key = (tuple(reals), dfr is not None)
        if key not in memo:
            memo[key] = _wave_pass(reals, place, dfr)
        return memo[key]

    out_chunks, dfr_chunks = [], []  # (pass, wave, entries)
    for w in range(waves):           # first launch: lanes take reads w * 64 + p * stride + lane
        left = n - w * 64
        reals = []
        while left > 0:
            reals.append(min(left, 64))
            left -= stride
        o, d = run(reals, defer)
        out_chunks += [(p, w, c) for p, c in o]
        dfr_chunks += [(p, w, c) for p, c in d]
    if defer:
        fill = [c for _, _, c in sorted(dfr_chunks)]  # the deferred list: a chunk holds its entries in front, holes behind
        res.update(defer_slots=K4_CHUNK * len(fill), deferred=sum(fill))
        segs = len(fill) * (K4_CHUNK // 64)
        for w in range(min(waves, segs)):  # second launch: the same grid over ctl[K4_CTL_DEFER] slots
            reals = [min(64, max(0, fill[sg // 8] - 64 * (sg % 8))) for sg in range(w, segs, waves)]
            o, _ = run(reals, None)
            out_chunks += [(p, w, c) for p, c in o]
    res.update(out_slots=K4_CHUNK * len(out_chunks), survivors=sum(c for _, _, c in out_chunks))
    return res


def later_step_slots(in_slots, in_real, n, nch, per_wave_survivors):
    """the worst placement of a step t >= 1 that walks in_slots slots holding in_real survivors, on the grid of the n-read batch"""
    bs = 128 if nch >= 16 else 256
    waves = min((n + bs - 1) // bs, 256 * 8 * (256 // bs)) * (bs // 64)
    s = min(in_real, _rate(per_wave_survivors)(64) * -(-in_real // 64))
    return K4_CHUNK * _worst_chunks(s, min(waves, -(-in_slots // 64)), -(-in_slots // (waves * 64)))


def fits(n, nch, split, reserved=None):
    """True when no share of survivors and of deferred reads in SHARES takes step 0, or the step behind it, of an n-read batch
    past the buffers a fresh handle reserves for it (or past `reserved` slots): what a GPU test asks before it sends the batch"""
    reserved = reserved_slots(n) if reserved is None else reserved
    for d in (SHARES if split else (None,)):
        for s in SHARES:
            m = slot_model(n, nch, 64 * s, None if d is None else 64 * d, placement="worst")
            nxt = later_step_slots(m["out_slots"], m["survivors"], n, nch, 64)
            if max(m["out_slots"], m["defer_slots"], nxt) > reserved:
                return False
    return True


# ---- what a test states about its index ----------------------------------------------------------------------------------------
def kmer_counts(chroms, k):
    """occurrences of every k-mer code (2 bits a base, first base highest) in the forward text of the entries; windows with a symbol
    above T are left out, so a k-mer table's bucket is at least this deep"""
    counts = np.zeros(4 ** k, dtype=np.int64)
    for c in chroms:
        c = np.asarray(c, dtype=np.int64)
        if len(c) < k:
            continue
        code = np.zeros(len(c) - k + 1, dtype=np.int64)
        ok = np.ones(len(c) - k + 1, dtype=bool)
        for j in range(k):
            w = c[j:len(c) - k + 1 + j]
            code = code * 4 + (w & 3)
            ok &= w <= 3
        counts += np.bincount(code[ok], minlength=4 ** k)
    return counts


def kmer_code(seq, k):
    v = 0
    for b in seq[:k]:
        v = v * 4 + int(b)
    return v


def kalign_core_offsets(rl, max_subs, min_core_len, max_num_slides, min_edit_dist=1):
    """offsets of every core that any AlignReads phase of a kalign read of rl bases places (k4d_read_params, k4d_read_plan and the
    core loop of k4d_lcm_fast, k4_align_common.h / k4_align.hip); min_core_len and max_num_slides as SfxIndex.min_core_len gives them"""
    mm = 0 if max_subs == 0 else min(63, max(1, int(0.5 + rl * max_subs / 100.0)))
    core = max(rl // (mm + 1 if min_edit_dist == 1 else mm + 2), min_core_len)
    sl = max(1, (max_num_slides * rl + 99) // 100)
    phases, t = [], 0
    while mm > 0 and t <= mm and rl // (t + min_edit_dist) > core:
        phases.append((rl // (t + min_edit_dist), rl // (t + min_edit_dist)))
        t += 1
    if mm == 0 or t <= mm:
        phases.append((core, max(rl // sl - 1, core)))
    offs = set()
    for cl, delta in phases:
        o, slides = 0, 0
        while slides < sl and o <= rl - cl and delta > cl // 3:
            if o + cl + delta > rl:
                delta = rl - (o + cl)
            offs.add(o)
            slides += 1
            o += delta
    return sorted(offs)


def never_probes_an_exception(reads, chroms, k, offsets):
    """per read: True when no suffix that begins with the first k bases of a core of the read (cores at `offsets`, either strand)
    lies where the read's window over the text would meet an N or an entry's end, to the 256-base blocks of the exception bitmap
    (K4_EXC_SHIFT).  The step kernels probe only suffixes of those k-mer buckets and hand a read whose window meets such a block
    to the general kernel, so these reads stay with them.  Reads of one length."""
    text = np.concatenate([np.concatenate([np.asarray(c, dtype=np.uint8), np.array([7], dtype=np.uint8)]) for c in chroms]).astype(np.int64)
    rl = len(reads[0])
    exc = np.concatenate([[0], np.cumsum(text > 3)])
    code = np.zeros(len(text) - k + 1, dtype=np.int64)
    for j in range(k):
        code = code * 4 + (text[j:len(text) - k + 1 + j] & 3)
    pos = np.nonzero(exc[k:] == exc[:-k])[0]  # k-mers of bases only
    pos = pos[np.argsort(code[pos], kind="stable")]
    sorted_codes = code[pos]
    fwd = np.stack([np.asarray(r, dtype=np.int64) for r in reads])
    ok = np.ones(len(reads), dtype=bool)
    for rd in (fwd, 3 - fwd[:, ::-1]):
        rc = np.zeros((len(reads), rl - k + 1), dtype=np.int64)
        for j in range(k):
            rc = rc * 4 + rd[:, j:rl - k + 1 + j]
        lo, hi = np.searchsorted(sorted_codes, rc, side="left"), np.searchsorted(sorted_codes, rc, side="right")
        cnt = (hi - lo).ravel()
        which = np.repeat(np.arange(cnt.size), cnt)               # (read, offset) of every occurrence
        occ = pos[np.repeat(lo.ravel(), cnt) + np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)]
        off = which % (rl - k + 1)
        start = occ - off                                         # where the read would lie
        b0 = np.maximum(start, 0) >> 8
        b1 = np.minimum(((start + rl - 1) >> 8) + 1, (len(text) + 255) >> 8)
        bad = (exc[np.minimum(b1 << 8, len(text))] != exc[b0 << 8]) & np.isin(off, offsets)
        ok[np.unique(which[bad] // (rl - k + 1))] = False
    return ok
