"""The seeded targets and crafted queries of the LocateQuerySeqs tests (numpy, CPU): tests/golden/make_golden_query.py runs the
reference over them, test_query_cpu.py the Python restatement, test_gpu_query.py the device.

targets(): seven targets, about 28 kb
  t1 6000, t3 3000, t4 3000   random (t3 and t4 lie next to one another in the concatenation)
  t2 5000                     random with an N run at 2000..2011
  t5 2000                     three 20-mers planted 4, 5 and 6 times (DEPTH_CORES; max_iter 5: max_iter - 1, max_iter, max_iter + 1)
  t6 1500                     a 37-base unit six times in tandem at 400, the fourth copy with one substitution
  t7 7000                     three 20-mers planted 63, 64 and 65 times (WAVE_CORES)
groups(): {group name: [(case name, query, params)]}, params = (core_len, core_delta, strand, max_hits, max_iter, match_pts, mismatch_pts)
"""
import numpy as np

SEED = 0x51525931
DFLT = (20, 10, 0, 1000, 100, 1, 3)
PARAM_NAMES = ("core_len", "core_delta", "strand", "max_hits", "max_iter", "match_pts", "mismatch_pts")
DEPTH_COUNTS = (4, 5, 6)
WAVE_COUNTS = (63, 64, 65)


def _rng(*k):
    return np.random.default_rng([SEED, *k])


def revcomp(q):
    q = np.asarray(q, dtype=np.uint8)[::-1].copy()
    m = q <= 3
    q[m] = 3 - q[m]
    return q


def _plant(t, cores, counts, gap, rng):
    pos = 30
    for c, n in zip(cores, counts):
        for _ in range(n):
            t[pos:pos + len(c)] = c
            pos += len(c) + gap + int(rng.integers(0, 5))
    assert pos < len(t)


def planted_cores():
    r = _rng(99)
    return [r.integers(0, 4, 20).astype(np.uint8) for _ in range(3)], [r.integers(0, 4, 20).astype(np.uint8) for _ in range(3)]


def targets():
    lens = (6000, 5000, 3000, 3000, 2000, 1500, 7000)
    ts = [_rng(1, i).integers(0, 4, n).astype(np.uint8) for i, n in enumerate(lens)]
    ts[1][2000:2012] = 4
    depth, wave = planted_cores()
    _plant(ts[4], depth, DEPTH_COUNTS, 25, _rng(2))
    _plant(ts[6], wave, WAVE_COUNTS, 12, _rng(3))
    unit = _rng(4).integers(0, 4, 37).astype(np.uint8)
    for k in range(6):
        ts[5][400 + 37 * k:437 + 37 * k] = unit
    ts[5][400 + 37 * 3 + 11] = (unit[11] + 1) % 4
    return ["q%d" % (i + 1) for i in range(len(ts))], ts


def _sub(q, positions):
    q = q.copy()
    for p in positions:
        q[p] = (q[p] + 1) % 4 if q[p] <= 3 else 0
    return q


def _junk(n, *k):
    return _rng(7, *k).integers(0, 4, n).astype(np.uint8)


def _p(**kw):
    p = list(DFLT)
    for k, v in kw.items():
        p[PARAM_NAMES.index(k)] = v
    return tuple(p)


def groups():
    _, ts = targets()
    t1, t2, t3, t4, t5, t6, t7 = ts
    depth, wave = planted_cores()
    g = {}
    # core walk: core_len 20, delta 7
    cw = []
    for ln in (20, 21, 27, 55, 56, 61):
        cw.append(("len%d" % ln, t1[100:100 + ln], _p(core_delta=7)))
    cw.append(("final_offset_only", np.concatenate([_junk(21, 1), t1[700:720]]), _p(core_delta=7)))
    cw.append(("last_probed_offset", np.concatenate([_junk(14, 2), t1[700:727]]), _p(core_delta=7)))
    g["corewalk"] = cw
    # extension
    copy = t1[1000:1400]
    ex = [("exact400", copy, DFLT)]
    pats = {"spaced50": list(range(25, 400, 50)), "burst5": [200, 201, 202, 203, 204], "every4th": list(range(150, 260, 4)),
            "every5th": list(range(150, 260, 5)), "dense": list(range(120, 200, 2)) + [300], "near_core": [21, 23, 25, 27, 380, 383, 386]}
    for nm, pos in pats.items():
        q = _sub(copy, pos)
        ex.append((nm, q, DFLT))
        ex.append((nm + "_rc", revcomp(q), DFLT))
        ex.append((nm + "_plus_only", q, _p(strand=1)))
        ex.append((nm + "_rc_minus_only", revcomp(q), _p(strand=2)))
        ex.append((nm + "_rc_plus_only", revcomp(q), _p(strand=1)))
    ex.append(("points_2_5", _sub(copy, pats["every5th"]), _p(match_pts=2, mismatch_pts=5)))
    ex.append(("targ_start", np.concatenate([_junk(50, 3), t3[:300]]), DFLT))
    ex.append(("targ_end", np.concatenate([t3[-300:], _junk(50, 4)]), DFLT))
    ex.append(("adjacent", np.concatenate([t3[-200:], t4[:200]]), DFLT))
    ex.append(("adjacent_rc", revcomp(np.concatenate([t3[-200:], t4[:200]])), DFLT))
    ex.append(("n_in_target", _sub(t2[1800:2200], [210]), DFLT))
    qn = t1[3000:3400].copy()
    qn[[5, 133, 290, 291]] = 4
    ex.append(("n_in_query", qn, DFLT))
    ex.append(("n_in_query_rc", revcomp(qn), DFLT))
    qn2 = t2[1900:2100].copy()  # N against N
    ex.append(("n_both", qn2, DFLT))
    g["extension"] = ex
    # containment and redundancy
    cr = []
    for d in (1, 2, 3):
        cr.append(("del%d" % d, np.concatenate([t1[2000:2200], t1[2200 + d:2400]]), DFLT))
        cr.append(("ins%d" % d, np.concatenate([t1[2000:2200], _junk(d, 5, d), t1[2200:2400]]), DFLT))
    cr.append(("tandem", np.concatenate([_junk(20, 6), t6[400:474], _junk(20, 7)]), _p(core_delta=5)))
    cr.append(("tandem_delta1", np.concatenate([_junk(20, 6), t6[437:548], _junk(20, 7)]), _p(core_delta=1)))
    cr.append(("swallowed", np.concatenate([t1[4000:4040], _junk(10, 8), t1[4040:4400]]), _p(core_delta=5)))
    cr.append(("swallowed_far", np.concatenate([t1[4000:4045], _junk(60, 9), t1[4045:4400]]), _p(core_delta=5)))
    g["redundancy"] = cr
    # depth
    dp = []
    for c, n in zip(depth, DEPTH_COUNTS):
        q = np.concatenate([c, _junk(1, 10)])
        dp.append(("planted%d_iter5" % n, q, _p(core_delta=1, max_iter=5)))
        dp.append(("planted%d_iter0" % n, q, _p(core_delta=1, max_iter=0)))
        dp.append(("planted%d_iter7" % n, q, _p(core_delta=1, max_iter=7)))
    g["depth"] = dp
    # caps and wave edges
    cp = []
    for c, n in zip(wave, WAVE_COUNTS):
        q = np.concatenate([c, _junk(1, 11)])
        cp.append(("occ%d" % n, q, _p(core_delta=1)))
    for mh in (1, 2, 3):
        cp.append(("max_hits%d" % mh, np.concatenate([wave[0], _junk(1, 11)]), _p(core_delta=1, max_hits=mh)))
        cp.append(("max_hits%d_both" % mh, np.concatenate([t1[1000:1100], revcomp(t3[500:600]), t4[100:200]]), _p(max_hits=mh)))
    for nc in (63, 64, 65, 129):
        ln = 20 + 10 * nc
        cp.append(("cores%d" % nc, _sub(t1[200:200 + ln], list(range(40, ln, 97))), DFLT))
    g["caps"] = cp
    return g


def batch():
    """lengths 0, 21 .. 20 000 in one batch: (queries, params)"""
    _, ts = targets()
    r = _rng(12)
    cat = np.concatenate(ts)
    qs = [np.zeros(0, np.uint8), ts[0][50:71], ts[0][50:70]]
    for ln in (64, 150, 999, 3000, 20000):
        s = int(r.integers(0, len(cat) - ln))
        q = cat[s:s + ln].copy()
        pos = r.choice(ln, size=ln // 50, replace=False)
        q[pos] = (q[pos] + 1 + r.integers(0, 3, len(pos))) % 4
        qs.append(revcomp(q) if ln == 999 else q)
    return qs, _p(max_hits=200)
