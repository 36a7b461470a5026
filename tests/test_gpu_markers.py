"""kalign's SNP centroids (-7) and marker sequences (-K) on the device (k4_snp_run2_dev: the centroid instance kernel with its LDS
histogram, the marker kernel with one wave per candidate) against the files `ngskit4b kalign` wrote (tests/golden/cent_* / mk_*) --
through the API on the device's own alignments and through `k4align` -- and against the Python restatement (tests/markers_ref.py)
on crafted stacks.  CKAligner::OutputSNPs, ngskit4b/KAligner.cpp:7380-7398, 7494-7560, 8104-8133, 8626-8660."""
import json
import os
import subprocess

import numpy as np
import pytest

import markers_ref
import pba_ref
import samutil
import synth
from test_markers_cpu import MARKER_CASES, golden_text, marker_args, snp_file_of
from test_oracle_sam_golden import kalign_args

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4ALIGN = os.path.join(ROOT, "kit4b_amd", "k4align")
SIDE = (("wig", ".covsegs.wig"), ("disnp", ".disnp.csv"), ("trisnp", ".trisnp.csv"))


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


@pytest.fixture(scope="module")
def aligned(k4, golden_dir):
    """{reads: (index, keywords of the alignments for snp_files)}: each read set aligned once, shared by its cases"""
    ix = k4.SfxIndex.open(os.path.join(golden_dir, "g1.sfx"))
    ix.set_max_iter(5000)
    out = {}
    snp_cases = json.load(open(os.path.join(golden_dir, "snp_cases.json")))
    for reads in sorted({m["reads"] for m in MARKER_CASES.values()}):
        kw, pe = kalign_args([a for a in snp_cases[reads]["args"] if a[:2] not in ("-p", "-P", "-1")])
        if reads.startswith("snp_pe"):
            _, r1 = samutil.read_fasta_xz(os.path.join(golden_dir, reads + "_1.fa.xz"))
            _, r2 = samutil.read_fasta_xz(os.path.join(golden_dir, reads + "_2.fa.xz"))
            out[reads] = ([x for p in zip(r1, r2) for x in p], dict(pe_recs=ix.kalign_pe_batch(r1, r2, **pe, **kw)))
        else:
            _, rd = samutil.read_fasta_xz(os.path.join(golden_dir, reads + ".fa.xz"))
            r = ix.kalign_ext_batch(rd, **kw) if "min_chimeric_len" in kw else ix.kalign_batch(rd, **kw)
            out[reads] = (rd, dict(out=r["out"], hits=r["hits"]))
    yield ix, out
    ix.close()


def golden_side_files(case):
    stem = MARKER_CASES[case]["reads"] if case.startswith("cent_") else case
    return {k: golden_text(stem + ext) for k, ext in SIDE}


@pytest.mark.parametrize("case", sorted(MARKER_CASES))
def test_every_file_through_the_api(aligned, case):
    ix, runs = aligned
    meta = MARKER_CASES[case]
    reads, recs = runs[meta["reads"]]
    files = ix.snp_files(reads, vcf=meta["ext"] == ".vcf", **recs, **marker_args(meta["args"]))
    want = snp_file_of(case)
    if meta["ext"] == ".vcf":  # (the header names the program and the index)
        keep = lambda t: [l for l in t.splitlines() if not l.startswith(("##source", "##reference"))]  # noqa: E731
        assert keep(files["snp"]) == keep(want)
    else:
        assert files["snp"] == want
    assert files["n_snps"] == meta["snps"]
    for k, text in golden_side_files(case).items():
        assert files[k] == text, k
    if "-7" in meta["args"]:
        assert files["centroids"] == golden_text(case + ".centroids.csv")
    if "markers" in meta:
        assert files["markers"] == golden_text(case + ".markers") and files["n_markers"] == meta["markers"]
    assert ("markers" in files) == ("markers" in meta) and ("centroids" in files) == ("-7" in meta["args"])


@pytest.mark.parametrize("case", sorted(MARKER_CASES))
def test_k4align_writes_the_reference_files(golden_dir, tmp_path, case):
    import lzma

    meta = MARKER_CASES[case]

    def unxz(name):
        dst = str(tmp_path / name[:-3])
        open(dst, "wb").write(lzma.open(os.path.join(golden_dir, name)).read())
        return dst

    reads = meta["reads"]
    inputs = ["-i", unxz(reads + "_1.fa.xz"), "-u", unxz(reads + "_2.fa.xz")] if reads.startswith("snp_pe") else ["-i", unxz(reads + ".fa.xz")]
    snp, cent = str(tmp_path / ("o" + meta["ext"])), str(tmp_path / "cent.csv")
    args = []
    for a in meta["args"]:
        args += ["-7", cent] if a == "-7" else [a]
    p = subprocess.run([K4ALIGN, "-I", os.path.join(golden_dir, "g1.sfx"), "-o", str(tmp_path / "o.sam"), "-S", snp] + args + inputs, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    keep = lambda t: [l for l in t.splitlines() if not l.startswith(("##source", "##reference"))]  # noqa: E731
    assert keep(open(snp).read()) == keep(snp_file_of(case))
    for k, text in golden_side_files(case).items():
        assert open(str(tmp_path / ("o" + dict(SIDE)[k]))).read() == text, k
    if "-7" in meta["args"]:
        assert open(cent).read() == golden_text(case + ".centroids.csv")
    else:
        assert not os.path.exists(cent)
    if "markers" in meta:
        assert open(snp + ".markers").read() == golden_text(case + ".markers")  # the name is appended to the SNP file's
        assert ("%d marker sequences" % meta["markers"]) in p.stderr
    else:
        assert not os.path.exists(snp + ".markers")


# ---- crafted stacks: alignments laid out as the device has them, on a small index of its own ----------------------------------------
def build_index(k4, chroms):
    import torch

    names = ["m%02d" % i for i in range(len(chroms))]
    seq = np.concatenate([np.concatenate([c, [7]]) for c in chroms]).astype(np.uint8)
    d_seq = torch.from_numpy(seq).cuda()
    sa = torch.empty(len(seq), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(seq), 4, d_seq.data_ptr(), sa.data_ptr())
    return k4.SfxIndex.from_device(len(seq), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(names, [len(c) for c in chroms]), keep=(sa, d_seq)), names


def lay_out(k4, alns):
    """(reads, results, hits) of accepted alignments [(chromosome, start, bases on the '+' strand)]; every other one on the '-' strand"""
    n = len(alns)
    hits, rr = np.zeros(n, k4.HIT_DTYPE), np.zeros(n, k4.RESULT_DTYPE)
    reads = []
    for i, (c, start, fwd) in enumerate(alns):
        minus = bool(i & 1)
        reads.append(synth.revcomp(fwd) if minus else fwd)
        hits[i] = (c + 1, start, len(fwd), ord("-") if minus else ord("+"), 0, 0)
        rr[i] = (1, 1, 0, 1, 1, 1)
    return reads, rr, hits


def tile(c, tgt, depth, holes=(), max_len=100, first=0, last=None):
    """`depth` layers of reads over tgt[first:last], each layer cut at other places; the first two layers leave the `holes` loci out"""
    alns = []
    last = len(tgt) if last is None else last
    for layer in range(depth):
        cuts = sorted(set(range(first + (layer * 17) % max_len, last, max_len)) | {first, last}
                      | ({h for h in holes} | {h + 1 for h in holes} if layer < 2 else set()))
        for a, b in zip(cuts[:-1], cuts[1:]):
            if not (layer < 2 and a in holes) and b > a:
                alns.append([c, a, tgt[a:b].copy()])
    return alns


def put(alns, c, locus, base, n=None):
    """the first n (all) reads of chromosome c that cover `locus` show `base` there"""
    k = 0
    for a in alns:
        if a[0] == c and a[1] <= locus < a[1] + len(a[2]) and (n is None or k < n):
            a[2][locus - a[1]] = base
            k += 1
    assert k == (n if n is not None else k) and k > 0, (c, locus, k)


def check_run(k4, chroms, alns, expect_called, **kw):
    """the run through the API against the restatement: the centroid file, the markers, the CSV's marker columns"""
    ix, names = build_index(k4, chroms)
    try:
        reads, rr, hits = lay_out(k4, [tuple(a) for a in alns])
        files = ix.snp_files(reads, out=rr, hits=hits, centroids=True, **kw)
    finally:
        ix.close()
    cnts = pba_ref.pileup(chroms, [tuple(a) for a in alns])
    ref = markers_ref.run(names, chroms, cnts, kw.get("min_snp_reads", 5), kw.get("snp_nonref_pcnt", 25.0), kw.get("marker_len", 0),
                          kw.get("marker_poly_thres", markers_ref.DFLT_POLY_THRES))
    called, cols = markers_ref.called_loci(files["snp"], names)
    assert len(called) == files["n_snps"] and set(expect_called) <= set(called), sorted(set(expect_called) - set(called))
    for c, l in called:
        assert l in ref["survivors"][c], (c, l)
    assert files["centroids"] == markers_ref.centroid_text(ref["insts"], chroms, cnts, called)
    if kw.get("marker_len"):
        assert files["markers"] == ref["markers"] and files["n_markers"] == ref["n_markers"]
        assert cols == {k: ref["ids"][k] for k in called}
    return files, ref


def other(b, k=1):
    return (int(b) + k) % 4


CENT_LENS = [1, 6, 7, 8, 2051, 101, 5003, 70003, 4097, 1050003]


def crafted_centroids():
    """sequences of 1, 6, 7 and 8 bases; covered loci at 2, 3, clen - 4 and clen - 3 only; an N at each of the seven window
    positions; a homopolymer (one bin takes every locus); a long sequence over many bins; lengths that are no multiple of the four
    loci of a thread or the 2048 of a tile; a sequence of more than 512 tiles, covered at its start and behind the 512th tile (a
    workgroup comes round to a second tile); homozygous substitutions, some without a 7-mer"""
    rng = np.random.default_rng(0xCE27)
    lens = CENT_LENS
    chroms = [rng.integers(0, 4, n).astype(np.uint8) for n in lens]
    chroms[5][50] = 4
    chroms[6][:] = 0
    alns = []
    for c in (0, 1, 2, 3, 5, 6, 7, 8):
        alns += tile(c, chroms[c], 6)
    for a, b in ((2, 4), (lens[4] - 4, lens[4] - 2)):  # m04: two loci at each end, nothing between
        alns += tile(4, chroms[4], 6, first=a, last=b)
    for a, b in ((100, 420), (512 * 2048 - 150, 512 * 2048 + 333), (lens[9] - 120, lens[9])):
        alns += tile(9, chroms[9], 6, first=a, last=b)
    snps = [(7, 1000), (7, 1003), (7, 3), (7, 2), (7, lens[7] - 4), (7, lens[7] - 3), (5, 47), (5, 60), (8, 4093), (6, 2500), (9, 512 * 2048 + 7)]
    for c, l in snps:
        put(alns, c, l, other(chroms[c][l]))
    return chroms, alns, snps


def claims_of_crafted_centroids(chroms, alns, snps):
    """what the input is built for, checked on the host before any device call; returns the restatement's run"""
    lens = CENT_LENS
    cnts = pba_ref.pileup(chroms, [tuple(a) for a in alns])
    ref = markers_ref.run(["m%02d" % i for i in range(len(lens))], chroms, cnts, 5, 25.0)
    cov4 = np.flatnonzero(cnts[4][0] + cnts[4][1])
    assert cov4.tolist() == [2, 3, lens[4] - 4, lens[4] - 3]
    idx = markers_ref.centroid_index
    assert [idx(chroms[c], l) is not None for c, l in ((0, 0), (1, 3), (2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (3, 5))] == [False, False, False, True, False, True, True, False]
    assert [idx(chroms[4], l) is not None for l in cov4] == [False, True, True, False]
    assert [idx(chroms[5], l) is None for l in range(46, 55)] == [False] + [True] * 7 + [False]
    assert ref["insts"][0] >= lens[6] - 6 and (ref["insts"] > 0).sum() > 12000
    assert all(l % 4 for l in lens[4:]) and lens[7] % 2048 and lens[7] > 34 * 2048 and lens[9] > 512 * 2048
    assert int((cnts[9][0] + cnts[9][1])[512 * 2048:].astype(bool).sum()) > 400
    assert sum(1 for c, l in snps if idx(chroms[c], l) is None) == 3
    return ref


def test_centroid_windows_bounds_and_bins(k4):
    chroms, alns, snps = crafted_centroids()
    ref = claims_of_crafted_centroids(chroms, alns, snps)
    files, _ = check_run(k4, chroms, alns, snps, min_snp_reads=5)
    rows = [l.split(",") for l in files["centroids"].splitlines()[1:]]
    assert sum(int(r[2]) for r in rows) == int(ref["insts"].sum()) and sum(int(r[3]) for r in rows) == files["n_snps"] - 3


MARKER_RUNS = [(25, None), (26, 0.5), (500, None)]


def crafted_markers(marker_len, thres):
    """candidates one locus inside and outside either end's flank; a coverage hole at the first, a middle and the last marker locus;
    a locus that needs the second allele; an N-majority locus; a half-and-half centre (with --markerpolythres 0.5 it calls the
    reference base); and a sequence with more candidates than one launch of the marker kernel takes"""
    rng = np.random.default_rng(0x3A2 + marker_len)
    m5 = marker_len // 2
    m3 = marker_len - 1 - m5
    gap = marker_len + 60
    clen = 12 * gap + 7
    chroms = [rng.integers(0, 4, clen).astype(np.uint8), rng.integers(0, 4, 5003).astype(np.uint8)]
    t = chroms[0]
    site = [m5 + gap * k for k in range(1, 10)]  # candidates far enough apart that no marker holds a neighbour's oddities
    holes = [site[0] - m5, site[1] + 1, site[2] + m3, site[3] - m5 - 1, site[3] + m3 + 1]  # the last two: just outside a marker
    alns = tile(0, t, 6, holes=holes)
    edge = [m5 - 1, m5, clen - 1 - m3, clen - m3]
    for l in edge + site[:4] + [site[7]]:
        put(alns, 0, l, other(t[l]))
    lo, hi = sorted((other(t[site[4]], 1), other(t[site[4]], 2)))  # site 4: one read shows the lower allele, five the higher one
    put(alns, 0, site[4], hi)
    put(alns, 0, site[4], lo, 1)
    put(alns, 0, site[5], 4)                      # site 5: every read N
    put(alns, 0, site[6], other(t[site[6]]), 3)   # site 6: three of six reads
    put(alns, 0, site[7] + 2, other(t[site[7] + 2]), 1)  # beside site 7: 1/6 non-reference, a polymorphic site of its marker
    # m01: forty layers, every locus with one substituted read -> more than 4096 candidates below 0.5; three real SNPs behind them
    d = chroms[1]
    many = tile(1, d, 40)
    seen = np.zeros(len(d), np.int64)
    for a in many:  # at locus l the (l mod 40)-th read that covers it is the substituted one
        for l in range(a[1], a[1] + len(a[2])):
            if seen[l] == l % 40:
                a[2][l - a[1]] = other(d[l])
            seen[l] += 1
    real = [4300, 4600, 4990 - m3 if marker_len < 100 else 4500]
    alns += many
    for l in real:
        put(alns, 1, l, other(d[l], 2))
    kw = dict(min_snp_reads=5, snp_nonref_pcnt=0.1, marker_len=marker_len)
    if thres is not None:
        kw["marker_poly_thres"] = thres
    # ---- what the input claims, on the host ----
    cnts = pba_ref.pileup(chroms, [tuple(a) for a in alns])
    ref = markers_ref.run(["m00", "m01"], chroms, cnts, 5, 0.1, marker_len, markers_ref.DFLT_POLY_THRES if thres is None else thres)
    gate = lambda c, l: markers_ref.marker_at(cnts[c], chroms[c], l, marker_len, 5, kw.get("marker_poly_thres", markers_ref.DFLT_POLY_THRES))  # noqa: E731
    assert [gate(0, l)[1] if gate(0, l)[0] is None else "ok" for l in edge] == ["start", "ok", "ok", "end"]
    assert [gate(0, l)[1] if gate(0, l)[0] is None else "ok" for l in site[:4]] == ["coverage", "coverage", "coverage", "ok"]
    seq, poly = gate(0, site[4])
    assert seq[m5] == "ACGT"[hi] and poly == 1 and cnts[0][2 + lo, site[4]] == 1
    seq, poly = gate(0, site[5])
    assert seq[m5] == "N" and poly == 0
    assert gate(0, site[6]) == (None, "centre" if thres == 0.5 else "allele")
    assert gate(0, site[7])[1] == 1
    assert len(ref["survivors"][1]) == 3 and sum(1 for c, _ in ref["ids"] if c == 1) == 3
    n_cand = int(((cnts[1][1] >= 1) & (cnts[1][0] + cnts[1][1] >= 5)).sum())
    assert n_cand > 4096 + 200 and sorted(real)[0] > 4096 + 100 and ref["rejects"]["proportion"] > 4096
    assert ref["n_markers"] == 2 + 1 + 3 + 3  # the inner two edge loci, site 3, sites 4, 5 and 7, m01's three
    return chroms, alns, [(0, edge[1]), (0, edge[2]), (0, site[3]), (0, site[7])] + [(1, l) for l in real], kw


@pytest.mark.parametrize("marker_len,thres", MARKER_RUNS, ids=["K25", "K26_t05", "K500"])
def test_marker_gate_on_crafted_stacks(k4, marker_len, thres):
    chroms, alns, expect, kw = crafted_markers(marker_len, thres)  # (its claims are checked inside, on the host)
    files, _ = check_run(k4, chroms, alns, expect, **kw)
    assert files["markers"].count(">Marker") == 9 and "|1\n" in files["markers"]


def test_no_alignment_gives_the_empty_table(k4):
    chroms = [np.random.default_rng(1).integers(0, 4, 300).astype(np.uint8)]
    ix, _ = build_index(k4, chroms)
    reads, rr, hits = lay_out(k4, [(0, 0, chroms[0][:100].copy())])
    rr["nar"] = 3
    files = ix.snp_files(reads, out=rr, hits=hits, centroids=True, marker_len=25)
    ix.close()
    assert files["n_snps"] == 0 and files["markers"] == "" and files["n_markers"] == 0
    rows = files["centroids"].splitlines()
    assert len(rows) == 16385 and rows[1] == '1,"AAAAAAA",0,0,"A",0,0,0,0,0,0' and rows[-1] == '16384,"TTTTTTT",0,0,"T",0,0,0,0,0,0'
