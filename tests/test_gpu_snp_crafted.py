"""kalign's SNP calling on the device (k4_snp_run_dev: pile-up, candidate kernel, coverage kernels, haplotype kernel, the host's
p-values, cut, slot assignment and texts) against the CPU oracle, file by file, on the crafted scenarios of tests/snp_craft.py:
chromosome ends of the background window, the candidate tests' equalities, read ends / separations / trims of the haplotype files,
the coverage forms and the WIG's bookkeeping, skipped alignments, the PE record form and the VCF form.
tests/test_snp_craft_cpu.py checks that the scenarios contain what they are built for."""
import pytest

import snp_craft
from test_gpu_markers import build_index
from test_oracle_snp import rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


@pytest.mark.parametrize("name,k", snp_craft.CASES, ids=["%s-%d" % c for c in snp_craft.CASES])
def test_every_file_against_the_oracle(k4, oracle, name, k):
    s = snp_craft.scenario(name)
    opts = s["opts"][k]
    want = snp_craft.oracle_files(oracle, s, k)
    ix, names = build_index(k4, s["chroms"])
    try:
        assert names == s["names"]
        if s["pe"]:
            files = ix.snp_files(s["pe_reads"], pe_recs=s["pe_recs"], vcf=s["vcf"], **opts)
        else:
            files = ix.snp_files(s["reads"], out=s["rr"], hits=s["hits"], vcf=s["vcf"], **opts)
        csv_alone = ix.snp_csv(s["reads"], out=s["rr"], hits=s["hits"], **opts) if (name, k) == ("thresholds", 0) else None
    finally:
        ix.close()
    if s["vcf"]:  # (the oracle writes the records only; the header names the program and the index)
        assert [l for l in files["snp"].splitlines() if not l.startswith("#")] == want["snp"].splitlines()
    else:
        assert files["snp"].splitlines()[0] == want["snp"].splitlines()[0]
        got_rows, got_ranks = rows(files["snp"])
        want_rows, want_ranks = rows(want["snp"])
        assert got_rows == want_rows
        assert sorted(got_ranks) == sorted(want_ranks)  # equal p-values have no defined order in the reference
    assert files["n_snps"] == want["n_snps"]
    assert files["wig"] == want["wig"]
    assert files["disnp"] == want["disnp"]
    assert files["trisnp"] == want["trisnp"]
    if csv_alone is not None:  # the entry point without the WIG and haplotype branches
        assert csv_alone == (files["snp"], files["n_snps"])
