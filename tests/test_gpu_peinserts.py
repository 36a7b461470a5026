"""kalign's per-target PE insert length distributions (`-3`) on the device: `k4align -3 -O` writes, byte for byte, the
<-O file>.peinserts.csv `ngskit4b kalign -3 -O` wrote (tests/golden/make_golden_peinserts.py), or none (SE), or an empty one (no read
accepted), and leaves the SAM and the three -O files as they are without it; SfxIndex.pe_insert_dist equals the restatement
(tests/peinserts_ref.py) array for array on synthetic k4_pe_read records: 1.2 M pairs on one target (the cap of a million pairs),
300 000 pairs over an index of 12 000 sequences (run boundaries everywhere, most targets empty), and 50 000 pairs with lone mates
(the shifted two-at-a-time pairing, the dropped last element)."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import peinserts_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
K4ALIGN = os.path.join(os.path.dirname(HERE), "kit4b_amd", "k4align")
CASES = json.load(open(os.path.join(GOLDEN, "peinserts_cases.json")))


def _unxz(tmp_path, name):
    dst = str(tmp_path / name[:-3])
    open(dst, "wb").write(lzma.open(os.path.join(GOLDEN, name)).read())
    return dst


def _stats_files(stem):
    return [stem + ".stats.csv", stem + ".stats.AlignCntsDist.csv", stem + ".stats.GlobalPEInsertDist.csv"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_k4align_writes_the_reference_file(tmp_path, case):
    meta = CASES[case]
    files = []
    for flag, r in zip(("-i", "-u"), meta["reads"]):
        files += [flag, _unxz(tmp_path, r)]
    cmd = [K4ALIGN, "-I", os.path.join(GOLDEN, meta["index"] + ".sfx")] + meta["args"] + files
    with3, plain = str(tmp_path / "with"), str(tmp_path / "plain")
    p = subprocess.run(cmd + ["-o", with3 + ".sam", "-O", with3 + ".stats.csv", "-3"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    made = with3 + ".stats.csv.peinserts.csv"
    if meta["file"] == "absent":
        assert not os.path.exists(made)
    elif meta["file"] == "empty":
        assert os.path.exists(made) and os.path.getsize(made) == 0
    else:
        assert open(made, "rb").read() == lzma.open(os.path.join(GOLDEN, "peinserts_%s.csv.xz" % case)).read()
    # the stage leaves the results alone: the SAM and the -O files are those of the run without -3
    p = subprocess.run(cmd + ["-o", plain + ".sam", "-O", plain + ".stats.csv"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert not os.path.exists(plain + ".stats.csv.peinserts.csv")
    assert open(with3 + ".sam", "rb").read() == open(plain + ".sam", "rb").read()
    for a, b in zip(_stats_files(with3), _stats_files(plain)):
        assert os.path.exists(a) == os.path.exists(b), a
        if os.path.exists(a):
            assert open(a, "rb").read() == open(b, "rb").read(), a


def test_a_failed_run_leaves_no_file(tmp_path):
    st = str(tmp_path / "x.csv")
    p = subprocess.run([K4ALIGN, "-I", os.path.join(GOLDEN, "g1.sfx"), "-o", str(tmp_path / "o.sam"), "-O", st, "-3", "-i", str(tmp_path / "missing_1.fa"),
                        "-u", str(tmp_path / "missing_2.fa")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and not os.path.exists(st) and not os.path.exists(st + ".peinserts.csv")


# ---- the device entry point on synthetic records ------------------------------------------------------------------------------------
def synthetic(rng, chrom, inserts, reject=0.05):
    """pairs in k4_pe_read layout: pair q on target chrom[q] with the ends `inserts[q]` apart (outer distance), 100-base reads, a fifth
    of the ends trimmed, PE1 on either side, ~reject of the pairs not accepted"""
    import kit4b_amd

    n = len(chrom)
    pe = np.zeros(2 * n, kit4b_amd.PE_READ_DTYPE)
    ok = np.repeat(rng.random(n) >= reject, 2)
    pe["nar"] = np.where(ok, 1, np.repeat(rng.integers(13, 19, n), 2))
    pe["num_hits"] = pe["inst"] = pe["pe_aligned"] = ok
    left = rng.integers(0, 100_000, n)
    first_left = rng.random(n) < 0.5  # PE1 is the left end
    h = pe["hit"]
    h["chrom_id"] = np.repeat(chrom, 2)
    h["match_len"] = 100
    h["match_loci"][0::2] = np.where(first_left, left, left + inserts - 100)
    h["match_loci"][1::2] = np.where(first_left, left + inserts - 100, left)
    h["strand"][0::2] = np.where(first_left, ord("+"), ord("-"))
    h["strand"][1::2] = np.where(first_left, ord("-"), ord("+"))
    trimmed = rng.random(2 * n) < 0.2
    h["reserved"] = np.where(trimmed, rng.integers(0, 12, 2 * n) | (rng.integers(0, 12, 2 * n) << 12) | (1 << 24), 0)
    return pe


def check_equal(ix, pe):
    import torch

    d_pe = torch.from_numpy(pe.view(np.uint8).copy()).cuda()
    got = ix.pe_insert_dist(len(pe) // 2, d_pe)
    want = R.collect(pe)
    for k in ("entry_id", "tot_pes", "median", "sum", "dist"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(d_pe.cpu().numpy(), pe.view(np.uint8))  # the records are only read
    return got


def test_a_million_pairs_of_one_target_are_counted():
    import kit4b_amd

    kit4b_amd.lib()
    rng = np.random.default_rng(0x3E70)
    n = 1_200_000
    # two narrow modes: the median lies between values that repeat ~10^5 times; the pairs behind the first million are all
    # long, so counting them would move every figure
    inserts = np.where(rng.random(n) < 0.5, rng.integers(180, 185, n), rng.integers(420, 425, n))
    inserts[1_050_000:] = 900
    pe = synthetic(rng, np.full(n, 1), inserts, reject=0.02)
    ix = kit4b_amd.SfxIndex.open(os.path.join(GOLDEN, "g1.sfx"))
    try:
        got = check_equal(ix, pe)
        assert got["entry_id"].tolist() == [1] and got["tot_pes"].tolist() == [1_000_000]
        assert int(got["dist"].sum()) == 1_000_000 and got["dist"][0, 51] == 0
        assert ix.pe_insert_dist(0, None)["entry_id"].size == 0
    finally:
        ix.close()


def test_12000_targets_most_of_them_empty():
    import torch

    import kit4b_amd as k4

    k4.lib()
    rng = np.random.default_rng(0x3E71)
    n_chrom = 12_000
    clens = rng.integers(120, 400, n_chrom)
    seq = np.concatenate([np.concatenate([rng.integers(0, 4, int(ln)).astype(np.uint8), [7]]) for ln in clens]).astype(np.uint8)
    d_seq = torch.from_numpy(seq).cuda()
    sa = torch.empty(len(seq), dtype=torch.int32, device="cuda")
    k4.build_sa_device(len(seq), 4, d_seq.data_ptr(), sa.data_ptr())
    ix = k4.SfxIndex.from_device(len(seq), 4, d_seq.data_ptr(), sa.data_ptr(), k4.make_entries(["t%05d" % i for i in range(n_chrom)], clens),
                                 keep=(sa, d_seq))
    try:
        n = 300_000
        live = rng.choice(n_chrom, 3000, replace=False) + 1  # a quarter of the targets; Zipf: one with a quarter of the pairs, a tail of 0..3
        w = 1.0 / np.arange(1, 3001) ** 1.3
        chrom = live[rng.choice(3000, n, p=w / w.sum())]
        pe = synthetic(rng, chrom, rng.integers(60, 800, n))
        got = check_equal(ix, pe)
        assert 1000 < len(got["entry_id"]) <= 3000 and (np.diff(got["entry_id"].astype(np.int64)) > 0).all()
        assert {1, 2, 3} <= set(got["tot_pes"].tolist()) and got["tot_pes"].max() > 10_000  # runs inside a wave, runs over many blocks
    finally:
        ix.close()


def test_lone_mates_shift_the_pairing():
    import kit4b_amd

    kit4b_amd.lib()
    rng = np.random.default_rng(0x3E72)
    n = 50_000
    pe = synthetic(rng, rng.integers(1, 4, n), rng.integers(60, 800, n))
    lone = np.flatnonzero((rng.random(2 * n) < 0.01) & (pe["nar"] == 1))  # ~2 % of the pairs lose one mate to a later stage (NoHit)
    if (int((pe["nar"] == 1).sum()) - len(lone)) % 2 == 0:
        lone = lone[:-1]
    pe["nar"][lone], pe["num_hits"][lone] = 2, 0
    order = R._sorted_reads(pe)
    assert len(order) % 2 == 1 and sum(order[k] // 2 != order[k + 1] // 2 for k in range(0, len(order) - 1, 2)) > 1000
    ix = kit4b_amd.SfxIndex.open(os.path.join(GOLDEN, "g1.sfx"))
    try:
        got = check_equal(ix, pe)
        assert got["entry_id"].tolist() == [1, 2, 3] and int(got["tot_pes"].sum()) == len(order) // 2
    finally:
        ix.close()
