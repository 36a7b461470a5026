"""kalign's per-target PE insert length table (`-3`) without a device: the library's median and column rules (k4_pe_insert_rule.h, the
functions the kernels run) against MedianInsertLen's loop as the reference has it, the restatement's two walks against each other
and against the reference's files (tests/golden/make_golden_peinserts.py), the text of k4_write_pe_insert_dist, and k4align's
argument rules."""
import ctypes as C
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import peinserts_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
K4ALIGN = os.path.join(os.path.dirname(HERE), "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "peinserts_cases.json")))


def median_loop(lens):
    """CKAligner::MedianInsertLen (KAligner.cpp:5256-5319), statement by statement, the inner loop included"""
    n = len(lens)
    if n == 0:
        return 0
    if n == 1:
        return lens[0]
    if n == 2:
        return ((lens[0] + lens[1]) & 0xFFFFFFFF) // 2
    lo = hi = 0
    for v in lens:
        if v < lo or lo == 0:
            lo = v
        if v > hi or hi == 0:
            hi = v
    if hi == lo:
        return hi
    for idx in range(1, n):
        cur = lens[idx]
        if cur < lo or cur > hi:
            continue
        under = over = 0
        for idy in range(n):
            if idy == idx or lens[idy] == cur:
                continue
            if lens[idy] < cur:
                under += 1
            else:
                over += 1
        if under == over:
            return cur
        if under < over:
            lo = cur
        else:
            hi = cur
    return ((lo + hi) & 0xFFFFFFFF) // 2


def test_median_twin_equals_the_loop():
    import kit4b_amd

    rng = np.random.default_rng(0x3E60)
    seen = dict(ties=0, flat=0, adjacent=0, first_unique=0, first_decides=0)
    for trial in range(4000):
        n = int(rng.integers(0, 51)) if trial % 40 else int(rng.integers(900, 1100))
        base = int(rng.integers(1, 700))
        width = int(rng.choice([1, 2, 3, 5, 12, 40]))  # narrow: ties, one value only, two adjacent values
        v = (base + rng.integers(0, width, n)).astype(np.uint32)
        if n > 3 and trial % 3 == 0:  # element 0 is the only one of its value, anywhere around the rest
            v[0] = base + int(rng.integers(-2, width + 2)) if base > 2 else base + width
            v[1:][v[1:] == v[0]] += 1
        lens = v.tolist()
        want = median_loop(lens) if n <= 60 else R.median_insert_len(lens)
        assert kit4b_amd.pe_insert_median_host(v) == want, lens
        assert R.median_insert_len(lens) == want
        if n > 2:
            seen["ties"] += len(set(lens)) < n
            seen["flat"] += len(set(lens)) == 1
            seen["adjacent"] += len(set(lens)) == 2
            seen["first_unique"] += lens.count(lens[0]) == 1
            seen["first_decides"] += lens.count(lens[0]) == 1 and median_loop_or(lens) != median_loop_or(lens[1:] + lens[:1])
    assert all(c >= 20 for c in seen.values()), seen
    big = np.array([0xFFFFFFF0, 0xFFFFFFF4, 0xFFFFFFF8, 0xFFFFFFFC], np.uint32)  # (Lo + Hi) / 2 wraps in 32 bits
    assert kit4b_amd.pe_insert_median_host(big) == median_loop(big.tolist())
    assert kit4b_amd.pe_insert_median_host(big[:2]) == median_loop(big[:2].tolist()) == 0x7FFFFFF2


def median_loop_or(lens):
    return median_loop(lens) if len(lens) <= 60 else R.median_insert_len(lens)


def test_columns():
    import kit4b_amd

    want = {0: 0, 99: 0, 100: 1, 108: 1, 109: 2, 590: 50, 598: 50, 599: 51, 600: 51, 601: 51, 0xFFFFFFFF: 51}
    for tlen, col in want.items():
        assert kit4b_amd.pe_insert_bin_host(tlen) == col == R.bin_of(tlen), tlen


def random_records(rng, n_pairs, n_chrom, lone=0.0, reject=0.1):
    import kit4b_amd

    pe = np.zeros(2 * n_pairs, kit4b_amd.PE_READ_DTYPE)
    chrom = np.repeat(rng.integers(1, n_chrom + 1, n_pairs), 2)
    ok = np.repeat(rng.random(n_pairs) >= reject, 2)
    pe["nar"] = np.where(ok, 1, 15)
    pe["pe_aligned"] = ok
    h = pe["hit"]
    h["chrom_id"] = chrom
    h["match_loci"] = np.repeat(rng.integers(0, 5000, n_pairs), 2) + rng.integers(0, 700, 2 * n_pairs)
    h["match_len"] = rng.integers(50, 151, 2 * n_pairs)
    h["strand"] = np.where(rng.random(2 * n_pairs) < 0.5, ord("+"), ord("-"))
    h["reserved"] = np.where(rng.random(2 * n_pairs) < 0.2, rng.integers(0, 20, 2 * n_pairs) | (rng.integers(0, 20, 2 * n_pairs) << 12), 0)
    gone = rng.random(2 * n_pairs) < lone  # a later stage took this mate out: its partner stays accepted and PE-aligned
    pe["nar"][gone & ok] = 2
    return pe


def test_the_two_walks_agree():
    rng = np.random.default_rng(0x3E61)
    for n_pairs, n_chrom, lone in ((0, 3, 0.0), (1, 1, 0.0), (400, 3, 0.0), (401, 7, 0.05), (900, 300, 0.03)):
        pe = random_records(rng, n_pairs, n_chrom, lone)
        rows, got = R.walk_literal(pe), R.collect(pe)
        assert len(rows) == len(got["entry_id"])
        for r, (chrom, num, med, tot, dist) in enumerate(rows):
            assert (chrom, num, med, tot) == (got["entry_id"][r], got["tot_pes"][r], got["median"][r], got["sum"][r])
            assert dist == got["dist"][r].tolist()
        if lone:  # the shifted pairing: elements of different pairs are taken together
            order = R._sorted_reads(pe)
            assert any(order[k] // 2 != order[k + 1] // 2 for k in range(0, len(order) - 1, 2))


def test_restatement_text_parses_the_reference_files():
    """the reference's own rows, parsed and printed again by the restatement's text(): header, column count and number format"""
    import synth

    names, chroms = synth.golden_genome()
    lens = [len(c) for c in chroms]
    for case, meta in CASES.items():
        if meta["file"] != "rows":
            continue
        want = lzma.open(os.path.join(GOLDEN, "peinserts_%s.csv.xz" % case), "rt").read()
        body = [l.split(",") for l in want.splitlines()[1:]]
        rows = dict(entry_id=np.array([names.index(f[0].strip('"')) + 1 for f in body]), tot_pes=np.array([int(f[2]) for f in body]),
                    median=np.array([int(f[3]) for f in body]),
                    sum=np.array([int(f[4]) * int(f[2]) for f in body]), dist=np.array([[int(x) for x in f[5:]] for f in body]))
        assert all(int(f[2]) == sum(int(x) for x in f[5:]) for f in body)
        assert R.text(rows, names, lens, 1) == want
    assert R.text(dict(entry_id=[]), names, lens, 0) == ""


# ---- the argument rules of k4align (no device is touched before they are checked) ---------------------------------------------------
def _run(*args):
    base = [K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-o", "/dev/null", "-i", os.path.join(GOLDEN, "names.fa")]
    return subprocess.run(base + list(args), capture_output=True, text=True, timeout=60)


SENTENCE = "PE insert length distributions requested but no output statistics file '-O<file>' specified"


@pytest.mark.parametrize("opt", ["-3", "--petranslendist"])
def test_pe_without_statistics_file(opt):
    p = _run("-u", os.path.join(GOLDEN, "names.fa"), opt)
    assert p.returncode == 1 and SENTENCE in p.stderr, p.stderr


def test_long_name_takes_no_value(tmp_path):
    # the option behind it is still read as an option: its own range check answers
    p = _run("-u", os.path.join(GOLDEN, "names.fa"), "-O", str(tmp_path / "s.csv"), "--petranslendist", "--siteprefsofs", "200")
    assert p.returncode == 1 and "must be in range -100..100" in p.stderr, p.stderr
    p = _run("-u", os.path.join(GOLDEN, "names.fa"), "-O", str(tmp_path / "s.csv"), "-3", "-9", "200")
    assert p.returncode == 1 and "must be in range -100..100" in p.stderr, p.stderr
    assert not os.path.exists(str(tmp_path / "s.csv.peinserts.csv"))


# (-r5, the fifth of -O's refusals, is not a paired-end mode in the first place)
@pytest.mark.parametrize("args", [["-b", "1"], ["-S", "0/2"], ["-G", "0,1"], ["-Z"]])
def test_inherits_the_refusals_of_the_statistics_file(tmp_path, args):
    p = _run("-u", os.path.join(GOLDEN, "names.fa"), "-O", str(tmp_path / "s.csv"), "-3", *args)
    assert p.returncode in (1, 3) and ("-O" in p.stderr) and "usage" not in p.stderr.lower(), p.stderr
    assert not os.path.exists(str(tmp_path / "s.csv.peinserts.csv"))


def test_se_run_accepts_and_ignores_it(tmp_path):
    # without -O as well: in single-end processing the option is off before the rule about -O is looked at
    for opt in ("-3", "--petranslendist"):
        p = _run(opt, "-9", "200")
        assert p.returncode == 1 and "must be in range -100..100" in p.stderr and SENTENCE not in p.stderr, p.stderr
        p = _run(opt, "-O", str(tmp_path / "s.csv"), "-9", "200")
        assert p.returncode == 1 and "must be in range -100..100" in p.stderr and SENTENCE not in p.stderr, p.stderr


def test_usage_names_the_option():
    p = subprocess.run([K4ALIGN], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "[-3 " in p.stderr


def test_abi():
    import kit4b_amd

    L = kit4b_amd.lib()
    want = {"k4_pe_insert_dist_dev": 5, "k4_free_pe_insert_dist": 1, "k4_write_pe_insert_dist": 4, "k4_pipeline_pe_insert_dist": 2,
            "k4_pe_insert_bin_host": 1, "k4_pe_insert_median_host": 3}
    assert set(want) <= set(kit4b_amd.ABI_SYMBOLS)
    for name, n in want.items():
        assert len(getattr(L, name).argtypes) == n, name
    assert C.sizeof(kit4b_amd.PeInsertDist) == 8 + 6 * C.sizeof(C.c_void_p)
