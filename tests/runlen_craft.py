"""Small indexes in which a chosen core occurs an exact number of times, at chosen ranks of its suffix-array run: the waves of the
search-call families walk a run 64 suffixes a turn, so a run of 63, 64, 65, 128 or 129 suffixes ends just before, at and just behind
a turn, and what decides the answer can be made to sit in the first lane of the first turn or the last lane of the last one.

An occurrence's rank inside the run is set by the four bases behind it (a base-4 number, code 0 sorts first, 255 last); a few random
bases separate the occurrences.  A random 24-mer does not turn up a second time in a few thousand random bases, nor does its reverse
complement; the tests compare with the restatements, which do not depend on that."""
import contextlib
import ctypes as C

import numpy as np

import query_ref

RUN_LENGTHS = (1, 63, 64, 65, 128, 129)


def _code(v):
    return np.array([(v >> 6) & 3, (v >> 4) & 3, (v >> 2) & 3, v & 3], dtype=np.uint8)


def _rand(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


@contextlib.contextmanager
def host_index(k4, oracle, names, chroms, dataset="runs"):
    """(SfxIndex.from_host over the oracle's suffix array, the restatements' (seq, sa, entries)), both closed on the way out"""
    h = oracle.build(names, chroms, dataset=dataset, threads=2)
    x = None
    try:
        el = oracle.el_size(h)
        sa_raw = np.ctypeslib.as_array(C.cast(oracle.L.k4o_sa_bytes(h), C.POINTER(C.c_uint8)), shape=(oracle.concat_len(h) * el,))
        x = k4.SfxIndex.from_host(np.array(oracle.seq(h)), sa_raw, el, k4.make_entries(names, [len(c) for c in chroms]), dataset=dataset)
        yield x, query_ref.index_from_oracle(oracle, h)
    finally:
        if x is not None:
            x.close()
        oracle.close(h)


def hamming_window(seed=31):
    """An entry of 33 000 random bases -- 32 768 + 213 K-mers of 20: one launch window of the Hammings kernel and a bit -- and a
    short second entry that holds the 150 bases around K-mer 32 768 with every 23rd base changed, so that the K-mers on both sides
    of the window's edge have Hammings of 1 and of 2 and more.  (names, chroms)"""
    rng = np.random.default_rng(seed)
    big = _rand(rng, 33000)
    near = big[32700:32850].copy()
    near[::23] = (near[::23] + 1) % 4
    return ["hamBig", "hamNear"], [big, np.concatenate([_rand(rng, 50), near, _rand(rng, 50)]).astype(np.uint8)]


def kmarkers_runs(r, seed=11):
    """Entry 1 (the target) and entries 2, 3 (foreign).  Two 24-mers, each exactly r times in the index: `first` has its one foreign
    occurrence (entry 2) at rank 0 of its run and r - 1 in the target behind it, `last` has it (entry 3) at rank r - 1 behind r - 1 in
    the target; with r = 1 the only occurrence is the target's.  `fork` occurs once, in the target, and shares its first 12 bases
    with `first`: a K-mer that survives to the prefix pass, whose prefix run is first's r occurrences and its own.
    (names, chroms, dict of the 24-mers)"""
    rng = np.random.default_rng(seed + r)
    first, last = _rand(rng, 24), _rand(rng, 24)
    fork = np.concatenate([first[:12], (first[12:] + 1 + _rand(rng, 12) % 3) % 4]).astype(np.uint8)

    def occ(m, v):
        return [m, _code(v), _rand(rng, 2)]

    target = [_rand(rng, 60)]
    n_t = r - 1 if r > 1 else 1
    for j in range(n_t):
        target += occ(first, 1 + j) + occ(last, j)
    target += [_rand(rng, 7), fork, _rand(rng, 60)]
    f2, f3 = [_rand(rng, 150)], [_rand(rng, 130)]
    if r > 1:
        f2 += occ(first, 0)
        f3 += occ(last, 255)
    f2.append(_rand(rng, 90))
    f3.append(_rand(rng, 110))
    chroms = [np.concatenate(p).astype(np.uint8) for p in (target, f2, f3)]
    return ["runT", "runF2", "runF3"], chroms, dict(first=first, last=last, fork=fork)


def zygosity_runs(r, seed=23):
    """Entry 1 holds a 25-base probe at offset 40; its first 12 bases occur exactly r times in the index, the other r - 1 spread over
    entries 2..4 as copies of the probe with none, one or two substitutions behind the core.  (names, chroms, probe, probe offset)"""
    rng = np.random.default_rng(seed + r)
    probe = _rand(rng, 25)
    src = np.concatenate([_rand(rng, 40), probe, _rand(rng, 80)]).astype(np.uint8)
    others = [[_rand(rng, 30 + 9 * e)] for e in range(3)]
    for j in range(r - 1):
        c = probe.copy()
        for s in range(j % 3):
            at = 12 + (5 * j + 6 * s) % 13
            c[at] = (c[at] + 1 + j % 3) % 4
        others[j % 3] += [c, _rand(rng, 5)]
    for o in others:
        o.append(_rand(rng, 40))
    chroms = [src] + [np.concatenate(o).astype(np.uint8) for o in others]
    return ["zygS", "zygA", "zygB", "zygC"], chroms, probe, 40
