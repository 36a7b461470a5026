"""genpba's packed base alleles on the device (k4_pba_run_dev: the pile-up SNP calling uses, one classification + coverage pass per
chromosome, the WIG walk on host threads) against the files `ngskit4b genpba` wrote (tests/golden/pba_*.pba.xz / .covsegs.wig.xz)
-- through the API on the device's own alignments and through `k4align -M3` -- and against the Python restatement (tests/pba_ref.py)
on crafted stacks and on synthetic alignments.  CKAligner::ProcessSNPs / OutputSNPs, ngskit4b/KAligner.cpp:8168-8575, 7194-7317."""
import lzma
import os
import subprocess

import numpy as np
import pytest

import pba_ref
import samutil
import synth
from test_oracle_sam_golden import kalign_args
from test_oracle_snp import trim_reads
from test_pba_cpu import PBA_CASES, golden_files

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4ALIGN = os.path.join(ROOT, "kit4b_amd", "k4align")


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


@pytest.mark.parametrize("case", sorted(PBA_CASES))
def test_pba_through_the_api(k4, golden_dir, case):
    import torch

    meta = PBA_CASES[case]
    kw, pe = kalign_args(meta["args"])
    ix = k4.SfxIndex.open(os.path.join(golden_dir, "g1.sfx"))
    ix.set_max_iter(5000)
    ids = dict(experiment_id=meta["clean_ids"][0], readset_id=meta["clean_ids"][1])
    if case.startswith("pba_pe"):
        _, r1 = samutil.read_fasta_xz(os.path.join(golden_dir, meta["reads"] + "_1.fa.xz"))
        _, r2 = samutil.read_fasta_xz(os.path.join(golden_dir, meta["reads"] + "_2.fa.xz"))
        out = ix.kalign_pe_batch(r1, r2, **pe, **kw)
        files = ix.pba([x for p in zip(r1, r2) for x in p], pe_recs=out, **ids)
    else:
        _, reads = samutil.read_fasta_xz(os.path.join(golden_dir, meta["reads"] + ".fa.xz"))
        nth = [int(a[2:]) for a in meta["args"] if a.startswith("-#")]
        reads = trim_reads(meta["args"], reads[::nth[0]] if nth else reads)  # -#<n>: every n-th read of the file, the first one included
        r = ix.kalign_ext_batch(reads, **kw) if "min_chimeric_len" in kw else ix.kalign_batch(reads, **kw)
        out, hits = r["out"], r["hits"]
        win = [int(a[2:]) for a in meta["args"] if a.startswith("-k")]
        if win:  # ReducePCRduplicates in front of the report
            d_rr = torch.from_numpy(out.view(np.int32).reshape(len(out), 6).copy()).cuda()
            d_hits = torch.from_numpy(hits.view(np.int32).reshape(len(out), -1).copy()).cuda()
            assert ix.reduce_pcr_dups(win[0], len(out), hits.shape[1], d_rr, d_hits) > 0
            out = d_rr.cpu().numpy().view(k4.RESULT_DTYPE).reshape(-1)
        files = ix.pba(reads, out=out, hits=hits, **ids)
    blob, wig = golden_files(case)
    assert files["pba"] == blob
    assert files["wig"] == wig
    assert files["n_chroms"] == meta["n_chroms"] == len(pba_ref.parse_pba(blob)[1])
    ix.close()


def unxz(golden_dir, tmp_path, name):
    dst = str(tmp_path / name[:-3])
    open(dst, "wb").write(lzma.open(os.path.join(golden_dir, name)).read())
    return dst


@pytest.mark.parametrize("case", sorted(PBA_CASES))
def test_k4align_writes_the_reference_pba(golden_dir, tmp_path, case):
    meta = PBA_CASES[case]
    if case.startswith("pba_pe"):
        files = ["-i", unxz(golden_dir, tmp_path, meta["reads"] + "_1.fa.xz"), "-u", unxz(golden_dir, tmp_path, meta["reads"] + "_2.fa.xz")]
    else:
        files = ["-i", unxz(golden_dir, tmp_path, meta["reads"] + ".fa.xz")]
    before = set(os.listdir(tmp_path))
    p = subprocess.run([K4ALIGN, "-I", os.path.join(golden_dir, "g1.sfx"), "-o", str(tmp_path / "o.pba"), "-M3", "--experimentid", meta["ids"][0],
                        "--readsetid=" + meta["ids"][1]] + meta["args"] + files, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    blob, wig = golden_files(case)
    assert open(str(tmp_path / "o.pba"), "rb").read() == blob
    assert open(str(tmp_path / "o.covsegs.wig")).read() == wig  # AppendFileNameSuffix: the extension of -o is replaced
    assert set(os.listdir(tmp_path)) - before == {"o.pba", "o.covsegs.wig"}  # no SAM, nothing else
    assert ("packed base alleles of %d sequences" % meta["n_chroms"]) in p.stderr


# ---- crafted stacks on g1: proportions that land exactly on the thresholds -----------------------------------------------------
# (stack size, {offset: number of reads carrying the same substitution there})
STACKS = [(20, {10: 3, 19: 4, 28: 5, 37: 6, 46: 7, 55: 8, 64: 14, 73: 15, 82: 16}), (8, {40: 6}), (5, {30: 1, 60: 2}), (4, {50: 3}), (3, {50: 1}),
          (2, {}), (1, {})]


def crafted_reads(chroms):
    """stacks of identical-position 100 bp reads on chr1 and chr3 (alternating strands), each read within five substitutions; a
    stack of six with one read N at offset 50; one read on chr4 (300 bases), none on chr2 and chr5; one read hanging over chr3's end"""
    rng = np.random.default_rng(0x9BA)
    reads, want = [], []  # want: (chromosome, locus, allele count, coverage) that must exist
    spots = [(0, 5000), (2, 3000), (0, 9000), (2, 7000), (0, 13000), (2, 11000), (0, 17000), (0, 21000)]
    for k, (size, subs) in enumerate(STACKS + [(6, {})]):
        c, start = spots[k]
        assert (chroms[c][start:start + 100] <= 3).all()
        stack = [chroms[c][start:start + 100].copy() for _ in range(size)]
        load = [0] * size
        for ofs, m in subs.items():
            alt = (int(stack[0][ofs]) + 1 + k % 3) % 4
            for j in sorted(range(size), key=lambda j: (load[j], j))[:m]:  # the reads with the fewest substitutions so far
                stack[j][ofs] = alt
                load[j] += 1
            want.append((c, start + ofs, m, size))
        assert max(load) <= 5
        if k == len(STACKS):
            stack[2][50] = 4  # a read N: coverage 5 there, 6 beside it
            want.append((c, start + 50, 5, 5))
        reads += [synth.revcomp(r) if k % 2 else r for r in stack]
    reads.append(chroms[3][200:300].copy())  # up to chr4's last base
    reads.append(np.concatenate([chroms[2][-60:], rng.integers(0, 4, 40).astype(np.uint8)]))  # over the end of chr3: no alignment lies there
    return reads, want


def test_crafted_stacks_against_the_restatement(golden_dir, tmp_path):
    names, chroms = synth.golden_genome()
    reads, want = crafted_reads(chroms)
    fa = str(tmp_path / "stacks.fa")
    synth.write_fasta(fa, reads)
    base = [K4ALIGN, "-I", os.path.join(golden_dir, "g1.sfx"), "-i", fa, "-s5"]
    p = subprocess.run(base + ["-o", str(tmp_path / "own.sam")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    p = subprocess.run(base + ["-o", str(tmp_path / "stacks"), "-M3", "--experimentid", "stacks", "--readsetid", "crafted"], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    recs = [l for l in open(str(tmp_path / "own.sam")).read().splitlines() if not l.startswith("@")]
    alns = pba_ref.sam_alignments(recs, names)
    assert len(alns) == len(reads) - 1  # every read but the one over chr3's end
    blob, wig, n_chroms, per = pba_ref.pba_files(names, chroms, alns, "stacks", "g1", "crafted")
    assert sorted(per) == [0, 2, 3]  # chr2 and chr5 hold no read: no record
    for c, locus, m, cov in want:  # the loci the stacks were built for are there
        cnt7 = per[c][0]
        assert per[c][2][locus] == cov and (cov == m or m in cnt7[2:6, locus]), (c, locus, m, cov)
    assert open(str(tmp_path / "stacks"), "rb").read() == blob
    assert open(str(tmp_path / "stacks.covsegs.wig")).read() == wig  # an -o without an extension: the suffix is appended
    # chr4's record: 300 bytes written to its end, the read's loci scored 2 (coverage 1 < 5), the others 0
    chr4 = dict(pba_ref.parse_pba(blob)[1])["chr4"]
    assert len(chr4) == 300 and (chr4[200:] != 0).all() and not chr4[:200].any()


# ---- the kernels' tails and the wider coverage forms: synthetic alignments on a small index -----------------------------------
# The classification and the coverage kernels take four loci per thread and 1024 per block.  g1's sequences (60000, 40000, 25000,
# 300, 120 bases) and g2's are all multiples of four: they cover residue 0 only.  The lengths below cover the residues 1, 2 and 3,
# sequences shorter than one thread's four loci, and lengths just below, at and above one and two blocks.
TAIL_LENS = [1, 2, 3, 5, 6, 7, 1021, 1022, 1023, 1024, 1025, 2047, 2049, 4093, 70003, 401]


@pytest.fixture(scope="module")
def small_index(k4):
    import torch

    rng = np.random.default_rng(0x9BA5)
    chroms = [rng.integers(0, 4, n).astype(np.uint8) for n in TAIL_LENS]
    for c in chroms[6:]:  # N runs, one of them at the very end of a sequence
        p = int(rng.integers(0, len(c) - 40))
        c[p:p + int(rng.integers(1, 40))] = 4
    chroms[8][-3:] = 4
    names = ["t%02d" % i for i in range(len(chroms))]
    seq = np.concatenate([np.concatenate([c, [7]]) for c in chroms]).astype(np.uint8)
    d_seq = torch.from_numpy(seq).cuda()
    sa = torch.empty(len(seq), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(seq), 4, d_seq.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(len(seq), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(names, TAIL_LENS), keep=(sa, d_seq))
    yield ix, names, chroms
    ix.close()


def synthetic(k4, chroms, skip, deep, seed):
    """alignment results laid out as the device has them and the restatement's (chromosome, start, '+' strand bases) list: reads of
    1..150 bases over every sequence but `skip`, both strands, trims, substitutions and read Ns, rejected reads, reads flagged as
    indels, reads reaching over their sequence's end; `deep`: (sequence, reads) stacks that push coverage past 255 / 65535"""
    rng = np.random.default_rng(seed)
    rows = []  # (chrom, start, length, minus, tl, tr, nar, ext)
    for c, tgt in enumerate(chroms):
        if c == skip:
            continue
        n_reads = max(4, len(tgt) // 12)
        for _ in range(n_reads):
            ln = int(min(rng.integers(1, 151), len(tgt)))
            start = int(rng.integers(0, len(tgt) - ln + 1))
            if len(tgt) > 200 and rng.random() < min(0.1, 20 / n_reads):
                start = len(tgt) - ln  # ends at the last locus (some twenty reads: the stack stays far below 256)
            tl, tr = (int(rng.integers(0, ln // 3 + 1)) if rng.random() < 0.2 else 0 for _ in range(2))
            rows.append((c, start, ln, rng.random() < 0.5, tl, tr, 1 if rng.random() < 0.9 else int(rng.integers(2, 9)),
                         (1 << 25) if rng.random() < 0.03 else 0))
        rows.append((c, max(len(tgt) - 3, 0), min(len(tgt), 3) + 5, False, 0, 0, 1, 0))  # over the end: skipped
    for c, n in deep:
        rows += [(c, 100, 120, bool(j & 1), 0, 0, 1, 0, j % 32) for j in range(n)]  # (32 different reads, each many times)
    n = len(rows)
    hits, rr = np.zeros(n, k4.HIT_DTYPE), np.zeros(n, k4.RESULT_DTYPE)
    reads, alns = [], []
    pool = {}
    for i, row in enumerate(rows):
        c, start, ln, minus, tl, tr, nar, ext = row[:8]
        tgt = chroms[c]
        if len(row) > 8 and (c, row[8]) in pool:
            fwd = pool[(c, row[8])]
        else:
            fwd = np.resize(tgt[start:start + ln], ln).copy()  # (an overhanging read repeats the sequence's end: its content is never looked at)
            fwd[fwd > 3] = rng.integers(0, 4)
            m = rng.random(ln) < 0.08
            fwd[m] = (fwd[m] + rng.integers(1, 4, int(m.sum()))) % 4
            fwd[rng.random(ln) < 0.02] = 4
            if len(row) > 8:
                pool[(c, row[8])] = fwd
        reads.append(synth.revcomp(fwd) if minus else fwd)
        hits[i] = (c + 1, start, ln, ord("-") if minus else ord("+"), 0, tl | (tr << 12) | ext)
        rr[i] = (1, 1, 0, 1, nar, 1 if nar == 1 else 0)
        if nar == 1 and not ext:
            lead, trail = (tr, tl) if minus else (tl, tr)  # the trims count from the read's own ends
            alns.append((c, start + lead, fwd[lead:ln - trail]))
    return reads, rr, hits, alns


@pytest.mark.parametrize("deep", [[], [(9, 300)], [(11, 70000), (10, 260)]], ids=["width1", "width2", "width4"])
def test_every_tail_and_coverage_width_against_the_restatement(k4, small_index, deep):
    ix, names, chroms = small_index
    skip = 7
    reads, rr, hits, alns = synthetic(k4, chroms, skip, deep, 0x7A11 + len(deep))
    files = ix.pba(reads, out=rr, hits=hits, experiment_id="tails", readset_id="w%d" % len(deep))
    blob, wig, n_chroms, per = pba_ref.pba_files(names, chroms, alns, "tails", "syn", "w%d" % len(deep))
    assert skip not in per and n_chroms == len(chroms) - 1
    mx = max(int(cov.max()) for _, _, cov in per.values())
    assert (mx < 256) if not deep else (256 <= mx < 65536) if len(deep) == 1 else (mx >= 65536)  # the coverage form the case is about
    assert files["n_chroms"] == n_chroms
    assert files["pba"] == blob
    assert files["wig"] == wig


def test_no_alignment_no_record(k4, small_index):
    ix, _, chroms = small_index
    reads, rr, hits, _ = synthetic(k4, chroms, 7, [], 0x7A10)
    rr["nar"] = np.where(rr["nar"] == 1, 3, rr["nar"])
    files = ix.pba(reads, out=rr, hits=hits, experiment_id="e", readset_id="r")
    assert files == {"pba": b"", "wig": "", "n_chroms": 0}  # the reference writes the header with its first chromosome
