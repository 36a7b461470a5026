"""Golden SNP centroid and marker files from the REAL reference front end (`oracle/_ref/ngskit4b kalign ... -7 <file>` /
`-K<len> [--markerpolythres <dbl>]`), on the read files the SNP goldens already have (tests/golden/make_golden_snp.py).

    python tests/golden/make_golden_markers.py

Centroid-only cases: `-7` added to the unchanged arguments of a SNP case; kept: the centroid CSV (xz).  Marker cases: kept are
the centroid CSV (xz, where -7 is given), <snp file>.markers, the SNP CSV / VCF, .disnp.csv, .trisnp.csv and .covsegs.wig (xz) --
with -K every one of them changes.  markers_cases.json: reads, arguments, marker count, SNP count.  Data only.

The generator refuses to write goldens that exercise nothing (the assertions in main)."""
import json
import lzma
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
NGS = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")
SNP_CASES = json.load(open(os.path.join(HERE, "snp_cases.json")))

# name: (reads / SNP case whose arguments are taken unchanged, extra arguments, extension of the SNP file)
CASES = {
    "cent_se": ("snp_se", ["-7"], ".csv"),
    "cent_se_c50_p8": ("snp_se_c50_p8", ["-7"], ".csv"),
    "cent_pe_hap_c60": ("snp_pe_hap_c60", ["-7"], ".csv"),
    "mk_se_hap_K25": ("snp_se_hap", ["-K25"], ".csv"),
    "mk_se_hap_K51_t02": ("snp_se_hap", ["-K51", "--markerpolythres", "0.2", "-7"], ".csv"),
    "mk_pe_hap_c60_K100": ("snp_pe_hap_c60", ["-K100", "-7"], ".csv"),
    "mk_se_K500": ("snp_se", ["-K500"], ".csv"),
    "mk_se_hap_K26_vcf": ("snp_se_hap", ["-K26"], ".vcf"),
}


def centroid_sums(text):
    rows = [l.split(",") for l in text.splitlines()[1:]]
    assert len(rows) == 16384
    return sum(int(r[2]) for r in rows), sum(int(r[3]) for r in rows)


def main():
    meta, polymorphic = {}, 0
    with tempfile.TemporaryDirectory() as tmp:
        for name, (reads, extra, ext) in CASES.items():
            files = []
            for flag, fn in (("-i", reads + "_1.fa.xz"), ("-u", reads + "_2.fa.xz")) if reads.startswith("snp_pe") else (("-i", reads + ".fa.xz"),):
                dst = os.path.join(tmp, fn[:-3])
                open(dst, "wb").write(lzma.open(os.path.join(HERE, fn)).read())
                files += [flag, dst]
            snp = os.path.join(tmp, name + ext)
            cent = os.path.join(tmp, name + ".centroids.csv")
            args = SNP_CASES[reads]["args"] + [a if a != "-7" else "-7" + cent for a in extra]
            # (the index by its bare name, from this directory: the VCF header's ##reference line repeats the -I argument)
            subprocess.run([NGS, "kalign", "-I", "g1.sfx", "-o", os.path.join(tmp, name + ".sam"), "-T", "4", "-F",
                            os.path.join(tmp, name + ".log"), "-S", snp] + args + files, check=True, capture_output=True, timeout=600, cwd=HERE)
            text = open(snp).read()
            n_snps = len([l for l in text.splitlines()[1:] if not l.startswith("#")])
            m = dict(reads=reads, args=SNP_CASES[reads]["args"] + extra, snps=n_snps, ext=ext)
            if "-7" in extra:
                ct = open(cent).read()
                insts, snps = centroid_sums(ct)
                assert snps > 0 and insts > snps, (name, insts, snps)
                with lzma.open(os.path.join(HERE, name + ".centroids.csv.xz"), "wb", preset=9) as g:
                    g.write(ct.encode())
                m["insts"], m["cent_snps"] = insts, snps
            if name.startswith("cent_"):  # -7 must not change calling: the committed SNP CSV of the case, byte for byte
                assert text == open(os.path.join(HERE, reads + ".csv")).read(), name
            else:
                mk = open(snp + ".markers").read()
                recs = [l for l in mk.splitlines() if l.startswith(">")]
                m["markers"] = len(recs)
                polymorphic += sum(1 for l in recs if int(l.rsplit("|", 1)[1]) > 0)
                if "-K500" not in extra:
                    assert len(recs) >= 20 and n_snps < SNP_CASES[reads]["snps"], (name, len(recs), n_snps)
                with lzma.open(os.path.join(HERE, name + ".markers.xz"), "wb", preset=9) as g:
                    g.write(mk.encode())
                open(os.path.join(HERE, name + ext), "w").write(text)
                stem = os.path.join(tmp, name)
                with lzma.open(os.path.join(HERE, name + ".covsegs.wig.xz"), "wb", preset=9) as g:
                    g.write(open(stem + ".covsegs.wig", "rb").read())
                for side in (".disnp.csv", ".trisnp.csv"):
                    open(os.path.join(HERE, name + side), "w").write(open(stem + side).read())
            meta[name] = m
            print(name, m)
    assert polymorphic > 0, "no marker with a polymorphic site in any case"
    json.dump(meta, open(os.path.join(HERE, "markers_cases.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    sys.exit(main())
