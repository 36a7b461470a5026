"""Golden packed base alleles from the REAL reference front end (`oracle/_ref/ngskit4b genpba -w<id> -W<id> -o x.pba`).

    make -C oracle ngskit4b && python tests/golden/make_golden_pba.py

The reads are the ones make_golden_snp.py drew (committed as snp_*.fa.xz); genpba aligns them to g1 as kalign does, piles the
accepted alignments up and writes one byte per locus (.pba) and the coverage WIG beside it.  Kept per case: the .pba and the
.covsegs.wig (xz), the command line (pba_cases.json) and -- where no SAM of `ngskit4b kalign` with the same alignment arguments is
committed yet -- that SAM (xz): the same CKAligner::Process, so the same accepted alignments.  Data only.

A case is written only when tests/pba_ref.py reproduces both files byte for byte from that SAM and the genome, and when all cases
together hold every 2-bit score 0..3 at loci with coverage >= 5 and every score 0..2 at covered loci below 5."""
import json
import lzma
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import pba_ref  # noqa: E402
import samutil  # noqa: E402
import synth  # noqa: E402

NGS = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")
SPECIES = "g1"
# reads: committed read set(s); sam: the committed kalign SAM of the same alignment arguments (None: made and committed here)
CASES = {
    # (the ids of the first case go through the front end's cleaning: quotes dropped, white space trimmed and reduced)
    "pba_se": dict(reads="snp_se", args=["-s3"], sam="snp_se", ids=[' golden  "exp" 1 ', "'rs one'"]),
    "pba_se_hap": dict(reads="snp_se_hap", args=["-s6"], sam="snp_se_hap", ids=["exp_hap", "rs_hap"]),
    "pba_se_c50": dict(reads="snp_se_c50_p8", args=["-s3", "-c50"], sam="snp_se_c50_p8", ids=["exp_c50", "rs_c50"]),
    "pba_pe_u1": dict(reads="snp_pe_u1", args=["-s3", "-U1", "-d200", "-D600"], sam="snp_pe_u1", ids=["exp_pe", "rs_pe"], pe=True),
    "pba_se_low": dict(reads="snp_se", args=["-s3", "-#4"], sam=None, ids=["exp_low", "rs_low"]),
    "pba_se_k20_y5": dict(reads="snp_se", args=["-s3", "-k20", "-y5", "-Y7"], sam=None, ids=["exp_k20", "rs_k20"]),
}


def unxz(name, tmp):
    dst = os.path.join(tmp, name[:-3])
    if not os.path.exists(dst):
        with lzma.open(os.path.join(HERE, name), "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
    return dst


def main():
    names, chroms = synth.golden_genome()
    meta, files, hist = {}, {}, np.zeros((2, 4), np.int64)  # hist[0]: coverage 1..4, hist[1]: coverage >= 5
    with tempfile.TemporaryDirectory() as tmp:
        for name, c in CASES.items():
            if c.get("pe"):
                inputs = ["-i", unxz(c["reads"] + "_1.fa.xz", tmp), "-u", unxz(c["reads"] + "_2.fa.xz", tmp)]
            else:
                inputs = ["-i", unxz(c["reads"] + ".fa.xz", tmp)]
            common = ["-I", os.path.join(HERE, "g1.sfx"), "-T", "4", "-F", os.path.join(tmp, name + ".log")] + c["args"] + inputs
            pba = os.path.join(tmp, name + ".pba")
            subprocess.run([NGS, "genpba", "-o", pba, "-w", c["ids"][0], "-W", c["ids"][1]] + common, check=True, capture_output=True, timeout=600)
            blob = open(pba, "rb").read()
            wig = open(os.path.join(tmp, name + ".covsegs.wig")).read()  # AppendFileNameSuffix: the extension is replaced
            sam_text = None
            if c["sam"]:
                _, recs = samutil.read_sam_xz(os.path.join(HERE, c["sam"] + ".sam.xz"))
            else:
                sam = os.path.join(tmp, name + ".sam")
                subprocess.run([NGS, "kalign", "-o", sam] + common, check=True, capture_output=True, timeout=600)
                sam_text = open(sam, "rb").read()
                recs = [l for l in sam_text.decode().splitlines() if not l.startswith("@")]
            hdr, got = pba_ref.parse_pba(blob)
            ids = [ln.split(":", 1)[1] for ln in hdr.split("\n")[2:]]
            want_blob, want_wig, n_chroms, per = pba_ref.pba_files(names, chroms, pba_ref.sam_alignments(recs, names), ids[0], SPECIES, ids[2])
            if want_blob != blob or want_wig != wig:
                raise SystemExit("%s: tests/pba_ref.py does not reproduce the reference (pba %s, wig %s): nothing written"
                                 % (name, want_blob == blob, want_wig == wig))
            for _, pb, cov in per.values():
                for sh in (6, 4, 2, 0):
                    s = (pb >> sh) & 3
                    hist[0] += np.bincount(s[(cov > 0) & (cov < 5)], minlength=4)
                    hist[1] += np.bincount(s[cov >= 5], minlength=4)
            files[name] = (blob, wig, sam_text)
            meta[name] = dict(args=c["args"], ids=c["ids"], clean_ids=[ids[0], ids[2]], reads=c["reads"], sam=c["sam"] or name, n_chroms=n_chroms,
                              pba_bytes=len(blob))
            print(name, meta[name])
    print("scores at coverage 1..4:", hist[0].tolist(), " at coverage >= 5:", hist[1].tolist())
    if not (hist[1] > 0).all() or not (hist[0][:3] > 0).all():
        raise SystemExit("not every score occurs in both coverage classes: nothing written (raise the sampling step of pba_se_low)")
    for name, (blob, wig, sam_text) in files.items():
        for ext, data in ((".pba.xz", blob), (".covsegs.wig.xz", wig.encode()), (".sam.xz", sam_text)):
            if data is not None:
                with lzma.open(os.path.join(HERE, name + ext), "wb", preset=9) as g:
                    g.write(data)
    json.dump(meta, open(os.path.join(HERE, "pba_cases.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
