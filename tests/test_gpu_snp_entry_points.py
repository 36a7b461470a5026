"""The five C entry points of SNP calling (k4_snp_csv_dev, k4_snp_vcf_dev, k4_snp_files_dev, k4_snp_run_dev, k4_snp_run2_dev) and
k4_pba_run_dev through the layers between them and the run: the same texts from every entry point that promises them (and the
oracle's, so that a shared mistake shows), nothing left in the caller's pointers or structs after a refused call, and the empty run.
One scenario: the haplotype stacks of tests/snp_craft.py (35 called SNPs, DiSNP and TriSNP lines, five sequences with coverage)."""
import ctypes as C

import pytest

import snp_craft
from test_gpu_markers import build_index

pytestmark = pytest.mark.gpu

ERR_PARAMS = -100
PATTERN = 0x5A5A5A5A5A5A5A5A
OPTS = (5, 0.05, 25.0)  # min_snp_reads, qvalue, snp_nonref_pcnt: snp_craft.DFLT
TRACK = 'track type=wiggle_0 name="Coverage" description="Alignment Segment Coverage" useScore=1\n'


@pytest.fixture(scope="module")
def k4():
    import kit4b_amd

    kit4b_amd.lib()  # raises if the HIP extension is missing: no fallback
    return kit4b_amd


@pytest.fixture(scope="module")
def run(k4):
    """the index of the scenario, its record arguments on the device and the callers of the six entry points"""
    s = snp_craft.scenario("haplotypes")
    ix, names = build_index(k4, s["chroms"])
    assert names == s["names"]
    rec, keep = ix._records(s["reads"], s["rr"], s["hits"], None)
    yield Calls(k4, ix, rec)
    del keep
    ix.close()


def filled(struct):
    """a ctypes struct with every byte set: what a refused call must have zeroed"""
    f = struct()
    C.memset(C.byref(f), 0x5A, C.sizeof(f))
    return f


def take(L, ptr, n):
    text = C.string_at(ptr, n).decode()
    L.k4_free_host(ptr)
    return text


class Calls:
    """each entry point as (return code, what it left with the caller): texts where it returned K4_OK (freed here), and the raw
    pointers and counts, which were pre-filled with a non-zero pattern"""

    def __init__(self, k4, ix, rec):
        self.k4, self.ix, self.rec, self.L = k4, ix, rec, k4.lib()

    def text(self, fn, rec, opts, vcf=None, wig=False):
        p = [C.c_void_p(PATTERN) for _ in range(2)]
        n = [C.c_uint64(PATTERN) for _ in range(3)]
        head = (self.ix.h,) + (() if vcf is None else (vcf,)) + tuple(rec) + tuple(opts)
        tail = (C.byref(p[1]), C.byref(n[2])) if wig else ()
        rc = fn(*head, C.byref(p[0]), C.byref(n[0]), C.byref(n[1]), *tail, 0)
        raw = [x.value or 0 for x in p[: 2 if wig else 1]] + [x.value for x in n[: 3 if wig else 2]]
        out = None
        if rc == 0:
            out = dict(snp=take(self.L, p[0], n[0].value), n_snps=n[1].value)
            if wig:
                out["wig"] = take(self.L, p[1], n[2].value)
        return rc, out, raw

    def csv(self, rec, opts):
        return self.text(self.L.k4_snp_csv_dev, rec, opts)

    def vcf(self, rec, opts):
        return self.text(self.L.k4_snp_vcf_dev, rec, opts)

    def files(self, rec, opts, vcf=0):
        return self.text(self.L.k4_snp_files_dev, rec, opts, vcf=vcf, wig=True)

    def struct_out(self, f, files, rc):
        raw = list(bytes(f))
        out = None
        if rc == 0:
            out = dict(n_snps=files.n_snps)
            for k in ("snp", "wig", "disnp", "trisnp"):
                out[k] = take(self.L, getattr(files, k), getattr(files, k + "_bytes"))
        return rc, out, raw

    def run(self, rec, opts, vcf=0):
        f = filled(self.k4.SnpFiles)
        rc = self.L.k4_snp_run_dev(self.ix.h, vcf, *rec, *opts, C.byref(f), 0)
        return self.struct_out(f, f, rc)

    def run2(self, rec, opts, vcf=0):
        f = filled(self.k4.SnpFiles2)
        o = self.k4.SnpOpts(0, 0, self.k4.DFLT_MARKER_POLY_THRES)
        rc = self.L.k4_snp_run2_dev(self.ix.h, vcf, *rec, *opts, C.byref(o), C.byref(f), 0)
        rc, out, raw = self.struct_out(f, f.files, rc)
        if out is not None:
            out.update(markers=f.markers, centroids=f.centroids, n_markers=f.n_markers)
        return rc, out, raw

    def pba(self, rec, ids=(b"e", b"r")):
        f = filled(self.k4.PbaFiles)
        rc = self.L.k4_pba_run_dev(self.ix.h, *rec, *ids, C.byref(f), 0)
        raw = list(bytes(f))
        out = None
        if rc == 0:
            out = dict(pba=C.string_at(f.pba, f.pba_bytes), n_chroms=f.n_chroms)
            self.L.k4_free_host(f.pba)
            out["wig"] = take(self.L, f.wig, f.wig_bytes)
        return rc, out, raw


@pytest.fixture(scope="module")
def full(run):
    """k4_snp_run_dev's files for vcf = 0 and 1: computed once, compared with by every test below"""
    res = {}
    for vcf in (0, 1):
        rc, res[vcf], _ = run.run(run.rec, OPTS, vcf)
        assert rc == 0
    return res


@pytest.fixture(scope="module")
def want(oracle):
    s = snp_craft.scenario("haplotypes")
    w = snp_craft.oracle_files(oracle, s, 0)
    w["vcf"] = snp_craft.oracle_files(oracle, dict(s, vcf=True), 0)["snp"]
    return w


def test_run_against_the_oracle(full, want):
    from test_oracle_snp import rows

    got_rows, got_ranks = rows(full[0]["snp"])
    want_rows, want_ranks = rows(want["snp"])
    assert full[0]["snp"].splitlines()[0] == want["snp"].splitlines()[0]
    assert got_rows == want_rows and sorted(got_ranks) == sorted(want_ranks)
    assert [l for l in full[1]["snp"].splitlines() if not l.startswith("#")] == want["vcf"].splitlines()
    for vcf in (0, 1):
        assert full[vcf]["n_snps"] == want["n_snps"] == 35
        assert full[vcf]["wig"] == want["wig"]
        assert full[vcf]["disnp"] == want["disnp"] and len(want["disnp"].splitlines()) == 17
        assert full[vcf]["trisnp"] == want["trisnp"]
    assert len(snp_craft.wig_spans(full[0]["wig"])) >= 2


def test_csv_and_vcf_alone(run, full):
    rc, out, _ = run.csv(run.rec, OPTS)
    assert rc == 0 and out == dict(snp=full[0]["snp"], n_snps=full[0]["n_snps"])
    rc, out, _ = run.vcf(run.rec, OPTS)
    assert rc == 0 and out == dict(snp=full[1]["snp"], n_snps=full[1]["n_snps"])


@pytest.mark.parametrize("vcf", [0, 1])
def test_files(run, full, vcf):
    rc, out, _ = run.files(run.rec, OPTS, vcf)
    assert rc == 0 and out == {k: full[vcf][k] for k in ("snp", "n_snps", "wig")}


@pytest.mark.parametrize("vcf", [0, 1])
def test_run2_without_options(run, full, vcf):
    rc, out, _ = run.run2(run.rec, OPTS, vcf)
    assert rc == 0 and out == dict(full[vcf], markers=None, centroids=None, n_markers=0)


@pytest.mark.parametrize("entry", ["csv", "vcf", "files", "run", "run2", "pba"])
@pytest.mark.parametrize("fault", ["option", "null_reads"])
def test_refused_call_leaves_nothing(run, entry, fault):
    """both are turned down by the argument checks, before anything is launched"""
    rec = list(run.rec)
    if fault == "null_reads":
        assert rec[1] > 0
        rec[6] = None  # d_reads
    if entry == "pba":
        rc, out, raw = run.pba(rec, ids=(None, b"r") if fault == "option" else (b"e", b"r"))
    else:
        rc, out, raw = getattr(run, entry)(rec, (0,) + OPTS[1:] if fault == "option" else OPTS)
    assert rc == ERR_PARAMS and out is None
    assert raw and not any(raw)


def test_empty_run(run):
    rec = list(run.rec)
    rec[1] = 0  # n_units
    csv_header = ('"SNP_ID","ElType","Species","Chrom","StartLoci","EndLoci","Len","Strand","Rank","PValue","Bases","Mismatches","RefBase",'
                  '"MMBaseA","MMBaseC","MMBaseG","MMBaseT","MMBaseN","BackgroundSubRate","TotWinBases","TotWinMismatches","MarkerID","NumPolymorphicSites"\n')
    snp_cols = lambda k: ",".join('"SNP%d%s"' % (k, x) for x in ("Loci", "RefBase", "BaseAcnt", "BaseCcnt", "BaseGcnt", "BaseTcnt", "BaseNcnt"))  # noqa: E731
    combos = lambda n: ",".join('"%s"' % "".join("acgt"[(q >> (2 * j)) & 3] for j in range(n - 1, -1, -1)) for q in range(4 ** n))  # noqa: E731
    di = '"DiSNPs_ID","ElType","Species","Chrom",%s,%s,"Depth","Antisense","Haplotypes",%s\n' % (snp_cols(1), snp_cols(2), combos(2))
    tri = '"TriSNPs_ID","ElType","Species","Chrom",%s,%s,%s,"Depth","Antisense","Haplotypes",%s\n' % (snp_cols(1), snp_cols(2), snp_cols(3), combos(3))
    assert di.startswith('"DiSNPs_ID","ElType","Species","Chrom","SNP1Loci","SNP1RefBase","SNP1BaseAcnt"') and di.endswith(',"tg","tt"\n')
    rc, out, _ = run.run(rec, OPTS)
    assert rc == 0 and out == dict(snp=csv_header, n_snps=0, wig=TRACK, disnp=di, trisnp=tri)
    rc, out, _ = run.run2(rec, OPTS)
    assert rc == 0 and out == dict(snp=csv_header, n_snps=0, wig=TRACK, disnp=di, trisnp=tri, markers=None, centroids=None, n_markers=0)
    rc, out, _ = run.files(rec, OPTS)
    assert rc == 0 and out == dict(snp=csv_header, n_snps=0, wig=TRACK)
    rc, out, _ = run.csv(rec, OPTS)
    assert rc == 0 and out == dict(snp=csv_header, n_snps=0)
    rc, out, _ = run.pba(rec)
    assert rc == 0 and out == dict(pba=b"", n_chroms=0, wig="")
