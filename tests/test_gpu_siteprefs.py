"""kalign's start-site octamer preferences (`-8`, `-9`) on the device: `k4align -8` writes, byte for byte, the file `ngskit4b kalign -8`
wrote (tests/golden/make_golden_siteprefs.py) and its SAM stays the reference's SAM; SfxIndex.site_prefs equals the restatement
(tests/siteprefs_ref.py) array for array on ~2 M synthetic alignments over a device-built index of 24 sequences with N runs."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import siteprefs_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
K4ALIGN = os.path.join(os.path.dirname(HERE), "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "siteprefs_cases.json")))


def _unxz(tmp_path, name):
    dst = str(tmp_path / name[:-3])
    open(dst, "wb").write(lzma.open(os.path.join(GOLDEN, name)).read())
    return dst


def _golden(case, ext):
    return lzma.open(os.path.join(GOLDEN, "siteprefs_%s.%s.xz" % (case, ext))).read()


def _sam(text):
    return [l for l in text.split("\n") if l and not l.startswith("@PG")]


def _inputs(tmp_path, meta):
    sfx = os.path.join(GOLDEN, "g1.sfx") if meta["index"] == "g1" else _unxz(tmp_path, meta["index"] + ".sfx.xz")
    files = []
    for flag, r in zip(("-i", "-u"), meta["reads"]):
        files += [flag, _unxz(tmp_path, r)]
    return sfx, files


@pytest.mark.parametrize("case", sorted(CASES))
def test_k4align_writes_the_reference_file(tmp_path, case):
    meta = CASES[case]
    sfx, files = _inputs(tmp_path, meta)
    out, site = str(tmp_path / "o.sam"), str(tmp_path / "o.site.csv")
    p = subprocess.run([K4ALIGN, "-I", sfx, "-o", out, "-8", site] + meta["args"] + files, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    for name, n in meta["nar"].items():
        assert ("%d (%s)" % (n, name)) in p.stderr, (name, n)
    assert open(site, "rb").read() == _golden(case, "csv")
    # the stage leaves the results alone: the SAM is the reference's, and the one of the run without -8
    assert _sam(open(out).read()) == _sam(_golden(case, "sam").decode())
    out2 = str(tmp_path / "plain.sam")
    args = [a for k, a in enumerate(meta["args"]) if a != "-9" and (k == 0 or meta["args"][k - 1] != "-9")]
    p = subprocess.run([K4ALIGN, "-I", sfx, "-o", out2] + args + files, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and open(out2, "rb").read() == open(out, "rb").read()


@pytest.mark.parametrize("extra", [["--chromexclude", "chr2"], ["-M1"], ["bam"], ["long"]])
def test_k4align_site_file_beside_other_outputs(tmp_path, extra):
    """-8 with a chromosome filter, -M1, BAM output and the long option names: the file is the restatement's over the SAM of that run
    (BAM, -M1: the same alignments as the plain run, the same file as the golden)"""
    import synth

    meta = CASES["se_default"]
    sfx, files = _inputs(tmp_path, meta)
    site = str(tmp_path / "o.site.csv")
    out = str(tmp_path / ("o.bam" if extra == ["bam"] else "o.sam"))
    opts = ["--siteprefs", site, "--siteprefsofs=-4"] if extra == ["long"] else ["-8", site] + (extra if extra[0].startswith("-") else [])
    p = subprocess.run([K4ALIGN, "-I", sfx, "-o", out] + opts + meta["args"] + files, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    if extra[0] == "--chromexclude":
        names, chroms = synth.golden_genome()
        recs = R.records_of_sam(open(out).read(), names)
        assert recs and all(r["chrom"] != 2 for r in recs)
        occ, sites = R.walk(recs, chroms, -4)
        assert open(site).read() == R.text(occ, sites, len(recs))
    else:
        assert open(site, "rb").read() == _golden("se_default", "csv")


def test_a_failed_run_leaves_no_site_file(tmp_path):
    site = str(tmp_path / "x.csv")
    p = subprocess.run([K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-o", str(tmp_path / "o.sam"), "-8", site, "-i", str(tmp_path / "missing.fa")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and not os.path.exists(site)


@pytest.mark.parametrize("args", [["-r5", "-R8"], ["-b", "1"], ["-S", "0/2"], ["-G", "0"], ["-Z"]])
def test_unsupported_combinations_exit_3_and_write_nothing(tmp_path, args):
    meta = CASES["se_none"]
    sfx, files = _inputs(tmp_path, meta)
    site, out = str(tmp_path / "s.csv"), str(tmp_path / "o.sam")
    p = subprocess.run([K4ALIGN, "-I", sfx, "-o", out, "-8", site] + args + files, capture_output=True, text=True, timeout=120)
    assert p.returncode == 3 and "not built" in p.stderr
    assert not os.path.exists(site) and not os.path.exists(out)


def test_offset_out_of_range_exits_1(tmp_path):
    meta = CASES["se_none"]
    sfx, files = _inputs(tmp_path, meta)
    for ofs in (["-9", "-101"], ["--siteprefsofs=101"]):
        p = subprocess.run([K4ALIGN, "-I", sfx, "-o", str(tmp_path / "o.sam"), "-8", str(tmp_path / "s.csv")] + ofs + files, capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 1 and "must be in range -100..100" in p.stderr and not os.path.exists(tmp_path / "s.csv")


# ---- the device entry point on synthetic alignments -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_index():
    """24 sequences with N runs, built on the device; the lengths put the sequences at every phase of a packed word"""
    import torch

    import kit4b_amd as k4

    k4.lib()
    rng = np.random.default_rng(0x5171)
    clens = np.concatenate([[9, 12, 12, 40], rng.integers(300, 3000, 20)])  # (two short ones: every locus is clamped to 3 on both)
    chroms = [rng.integers(0, 4, int(ln)).astype(np.uint8) for ln in clens]
    for c in chroms[4:]:  # (the four short ones hold no N)
        for _ in range(3):
            p = int(rng.integers(0, len(c) - 40))
            c[p:p + int(rng.integers(1, 40))] = 4
    chroms[5][40:120] = rng.integers(0, 4, 80)  # (the hot site of synthetic() holds no N)
    seq = np.concatenate([np.concatenate([c, [7]]) for c in chroms]).astype(np.uint8)
    d_seq = torch.from_numpy(seq).cuda()
    sa = torch.empty(len(seq), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(seq), 4, d_seq.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(len(seq), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(["t%02d" % i for i in range(24)], clens), keep=(sa, d_seq))
    yield ix, chroms
    ix.close()


def synthetic(chroms, n, seed, pe=False):
    """n results in load order (device-layout arrays) and the restatement's columns in walk order: both strands, lengths 36..300,
    ~8 % rejected, ~3 % two-segment and ~15 % trimmed reads; starts over the whole of every sequence (all 16 phases, sequence ends,
    N runs), a tenth of them within the first and last 120 bases (clamp, wrap-then-clamp, the undefined range); stacks of equal
    reads; half of all reads on ONE site of sequence 5 (the contention path)"""
    import kit4b_amd as k4

    rng = np.random.default_rng(seed)
    clens = np.array([len(c) for c in chroms], np.int64)
    chrom = rng.integers(0, len(chroms), n)
    lens = np.minimum(rng.integers(36, 301, n), clens[chrom])
    start = (rng.random(n) * (clens[chrom] - lens + 1)).astype(np.int64)
    edge = rng.random(n) < 0.1
    start = np.where(edge & (rng.random(n) < 0.5), np.minimum(rng.integers(0, 120, n), clens[chrom] - lens), start)
    start = np.where(edge & (start > 120), np.maximum(clens[chrom] - lens - rng.integers(0, 20, n), 0), start)
    dup = rng.random(n) < 0.3  # stacks: a read repeats the one in front of it (same site, another load position)
    dup[0] = False
    src = np.arange(n)
    src[dup] = 0
    src = np.maximum.accumulate(src)
    chrom, lens, start = chrom[src], lens[src], start[src]
    minus = (rng.random(n) < 0.5)[src]
    hot = rng.random(n) < 0.5
    chrom[hot], start[hot], lens[hot], minus[hot] = 5, 64, 100, False
    tl = np.where(rng.random(n) < 0.15, rng.integers(0, 20, n), 0)
    tr = np.where(rng.random(n) < 0.15, rng.integers(0, 20, n), 0)
    tl, tr = np.minimum(tl, lens // 3), np.minimum(tr, lens // 3)
    segs = rng.random(n) < 0.03
    mm = rng.integers(0, 4, n)
    nar = np.where(rng.random(n) < 0.08, rng.integers(2, 9, n), 1)
    hits = np.zeros(n, k4.HIT_DTYPE)
    hits["chrom_id"], hits["match_loci"], hits["match_len"], hits["mismatches"] = chrom + 1, start, lens, mm
    hits["strand"] = np.where(minus, ord("-"), ord("+"))
    hits["reserved"] = tl | (tr << 12) | np.where(segs, 1 << 25, 0)
    if pe:
        rr = np.zeros(n, k4.PE_READ_DTYPE)
        rr["nar"], rr["num_hits"], rr["hit"] = nar, nar == 1, hits
    else:
        rr = np.zeros(n, k4.RESULT_DTYPE)
        rr["nar"], rr["num_hits"], rr["hit_rslt"], rr["inst"] = nar, nar == 1, 1, 1
    acc = np.flatnonzero(nar == 1)
    adj = start + np.where(minus, tr, tl)
    order = acc[np.lexsort((acc, mm[acc], minus[acc], (lens - tl - tr)[acc], adj[acc], chrom[acc]))]  # SortHitMatch, ties in load order
    cols = (chrom[order] + 1, start[order], lens[order], minus[order], segs[order])
    return rr, hits, cols, int(len(acc))


def _check(ix, chroms, n, seed, ofs, pe=False):
    import torch

    rr, hits, cols, n_acc = synthetic(chroms, n, seed, pe)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()  # noqa: E731
    d_rr, d_hits = dev(rr), dev(hits)
    got = ix.site_prefs(n, 1, ofs, d_pe=d_rr) if pe else ix.site_prefs(n, 1, ofs, d_rr=d_rr, d_hits=d_hits)
    occ, sites = R.walk_arrays(*cols, chroms, ofs)
    assert got["n_accepted"] == n_acc
    assert got["n_counted"] == occ.sum() > 0
    assert np.array_equal(got["num_occs"], occ) and np.array_equal(got["num_sites"], sites)
    assert np.array_equal(d_rr.cpu().numpy(), rr.view(np.uint8)) and np.array_equal(d_hits.cpu().numpy(), hits.view(np.uint8))  # untouched
    return got, occ, sites


def test_device_counts_equal_the_restatement_2m_reads(small_index):
    ix, chroms = small_index
    got, occ, sites = _check(ix, chroms, 2_000_000, 0x5172, -4)
    assert occ[0].max() > 800_000            # one octamer draws half of all reads
    assert (occ[1] > 0).sum() > 5_000 and (sites > 1).sum() > 1_000
    # the literal walk over a slice of the same kind agrees with the numpy form the 2 M are held against
    rr, hits, cols, _ = synthetic(chroms, 30_000, 0x5173)
    recs = [dict(chrom=int(c), loci=int(l), mlen=int(m), strand="-" if s else "+", segs=bool(g)) for c, l, m, s, g in zip(*cols)]
    o1, s1 = R.walk(recs, chroms, -4, skip_undefined=True)
    o2, s2 = R.walk_arrays(*cols, chroms, -4)
    assert np.array_equal(o1, o2) and np.array_equal(s1, s2)
    with pytest.raises(R.Undefined):         # (the set does hold reads in the undefined range)
        R.walk(recs, chroms, -4)


@pytest.mark.parametrize("ofs,pe,hist", [(-100, False, "atomic"), (100, False, "atomic"), (0, True, "atomic"), (-4, False, "sort"), (7, True, "sort")])
def test_device_counts_offsets_pe_and_both_histogram_forms(small_index, monkeypatch, ofs, pe, hist):
    ix, chroms = small_index
    monkeypatch.setenv("K4_SITEPREFS_HIST", hist)
    _check(ix, chroms, 300_001, 0x5174 + ofs, ofs, pe)


def test_empty_call_nothing_accepted_and_bad_offset(small_index):
    import torch

    import kit4b_amd as k4

    ix, chroms = small_index
    got = ix.site_prefs(0, 1, -4)
    assert got["n_accepted"] == 0 and not got["num_occs"].any() and not got["num_sites"].any()
    rr, hits, _, _ = synthetic(chroms, 5000, 0x5175)
    rr["nar"] = 3
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()  # noqa: E731
    d_rr, d_hits = dev(rr), dev(hits)
    got = ix.site_prefs(5000, 1, -4, d_rr=d_rr, d_hits=d_hits)
    assert got["n_accepted"] == 0 and got["n_counted"] == 0 and not got["num_occs"].any()
    for ofs in (-101, 101):
        with pytest.raises(k4.K4Error) as e:
            ix.site_prefs(5000, 1, ofs, d_rr=d_rr, d_hits=d_hits)
        assert e.value.code == -100
