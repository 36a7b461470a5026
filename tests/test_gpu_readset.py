"""What each rejecting stage leaves in a read's record: nar, num_hits, inst and low_mm of every record behind the loci constraints,
the chromosome filter, the 5' primer correction (SE and PE record form each) and auto-trim (SE), on 64 crafted reads / 32 crafted
pairs over tests/golden/g1.sfx.  The stages clear different fields (DESIGN.md "Where a stage reads and rejects records"); the SAM
body shows none of that.

tests/golden/readset_stage_marks.json was recorded on an MI355X from the commit before the stages moved onto the shared record
view (K4ReadSet): stage_records() below, run against that commit's library, written out with json.dump."""
import json
import os

import numpy as np
import pytest

import primer_craft
import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_SE, N_PAIRS = 64, 32
FIELDS = ("nar", "num_hits", "inst", "low_mm")
NAR_OF = {"loci": 19, "chroms": 11, "primer": 3, "trim": 6}  # the NAR each stage gives a read it rejects


def _dev(a, pad=0):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    return torch.cat([t, torch.zeros(pad, dtype=torch.uint8, device="cuda")]) if pad else t


def _fields(rec):
    return {k: rec[k].astype(int).tolist() for k in FIELDS}


def stage_records(ix, chroms):
    """{"<stage>_<se|pe>": {"before": fields, "after": fields}}: every stage on a fresh copy of the same crafted records"""
    import kit4b_amd

    out = {}
    # loci constraints: sequence 1 has to read A wherever a read lies on it; chromosome filter: sequence 2 is refused
    table = np.zeros(1, kit4b_amd.LOCI_CONSTRAINT_DTYPE)
    table[0]["chrom_id"], table[0]["start"], table[0]["end"], table[0]["bits"] = 1, 0, len(chroms[0]) - 1, 0x01
    accept = np.ones(len(chroms) + 1, np.uint8)
    accept[0], accept[2] = 0, 0
    for form, n, seed in (("se", N_SE, 0x5E70), ("pe", 2 * N_PAIRS, 0x5E71)):
        s = primer_craft.craft(chroms, n, seed)
        s["rr"]["inst"] = np.where(s["rr"]["nar"] == 1, 3, 0)  # (a value no stage writes: a cleared LowHitInstances shows)

        def fresh():
            d = dict(reads=_dev(s["reads"], 64), offs=_dev(s["offs"]), lens=_dev(s["lens"]))
            if form == "se":
                d["rec"] = dict(d_rr=_dev(s["rr"]), d_hits=_dev(s["hits"]))
            else:
                d["rec"] = dict(d_pe=_dev(primer_craft.as_pe(s["rr"], s["hits"])))
            return d

        def back(d):
            if form == "se":
                return d["rec"]["d_rr"].cpu().numpy().view(primer_craft.RESULT_DTYPE)
            return d["rec"]["d_pe"].cpu().numpy().view(primer_craft.PE_READ_DTYPE)

        before = _fields(s["rr"])
        d = fresh()
        ix.filter_loci_constraints(table, n if form == "se" else n // 2, 1, d["reads"], d["offs"], d["lens"], **d["rec"])
        out["loci_" + form] = dict(before=before, after=_fields(back(d)))
        d = fresh()
        ix.filter_chroms(_dev(accept), n, 1, **d["rec"])
        out["chroms_" + form] = dict(before=before, after=_fields(back(d)))
        d = fresh()
        ix.pcr5_primer_correct(1, n, 1, d["reads"], d["offs"], d["lens"], **d["rec"])
        out["primer_" + form] = dict(before=before, after=_fields(back(d)))
        if form == "se":
            reads = s["reads"].copy()  # every fourth read differs from its target at every third base: no flank of 8 exact bases
            for i in range(0, n, 4):
                o = int(s["offs"][i])
                reads[o:o + int(s["lens"][i]):3] ^= 1
            rr, _, _ = ix.post_stages((reads, s["offs"], s["lens"]), s["rr"], s["hits"].reshape(n, 1), np.zeros(n, kit4b_amd.SEG2_DTYPE),
                                      min_flank_exacts=8)
            out["trim_se"] = dict(before=before, after=_fields(rr))
    return out


def test_every_rejecting_stage_leaves_the_recorded_fields():
    import kit4b_amd

    kit4b_amd.lib()
    assert kit4b_amd.RESULT_DTYPE == primer_craft.RESULT_DTYPE and kit4b_amd.PE_READ_DTYPE == primer_craft.PE_READ_DTYPE
    with open(os.path.join(GOLDEN, "readset_stage_marks.json")) as f:
        want = json.load(f)
    _, chroms = synth.golden_genome()
    ix = kit4b_amd.SfxIndex.open(os.path.join(GOLDEN, "g1.sfx"))
    try:
        got = stage_records(ix, chroms)
    finally:
        ix.close()
    assert sorted(got) == sorted(want) == sorted(["loci_se", "loci_pe", "chroms_se", "chroms_pe", "primer_se", "primer_pe", "trim_se"])
    for name in sorted(want):
        b, a = want[name]["before"], want[name]["after"]
        n = N_SE if name.endswith("_se") else 2 * N_PAIRS
        assert all(len(b[k]) == n and len(a[k]) == n for k in FIELDS), name
        assert got[name]["before"] == b, name  # the same inputs as the recorded run's
        # not vacuous, in the recorded run and in this one: the stage rejects accepted reads with its NAR and NumHits 0, and keeps some
        for after in (a, got[name]["after"]):
            was = np.array(b["nar"]) == 1
            rejected = was & (np.array(after["nar"]) == NAR_OF[name.split("_")[0]])
            kept = was & (np.array(after["nar"]) == 1)
            assert rejected.sum() >= 1 and kept.sum() >= 1, (name, int(rejected.sum()), int(kept.sum()))
            assert (np.array(after["num_hits"])[rejected] == 0).all(), name
            if name == "trim_se":  # AutoTrimFlanks' MatchLen != ReadLen branch: NumHits 0 under an unchanged NAR
                assert (kept & (np.array(after["num_hits"]) == 0)).sum() >= 1
        for k in FIELDS:
            assert got[name]["after"][k] == a[k], (name, k)
