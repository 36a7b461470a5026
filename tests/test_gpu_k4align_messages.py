"""What `k4align` says and how it ends: exit code, stderr lines and the files it leaves, for one run of every mode and for the
early refusals and failed opens that leave the run between the opening of the index and the first output.  The SAM / BAM / report
bytes are pinned elsewhere (test_gpu_io.py and the stage tests); the goldens there do not see stderr or a failing path's exit code.

tests/golden/k4align_messages.json was recorded on an MI355X from the commit before k4align's run function was broken up into
steps over one run state with one owner for its handles (tests/golden/make_golden_k4align_messages.py, which runs record() below
against that commit's binary).  Every `%.2fs` figure and the byte count of the compressed BAM are masked; all else is compared
as it is.  The runs use relative file names from a directory of their own, so no line holds a path of the machine.

Four of the failure cases (refuse_r3_b, refuse_a_S, missing_reads, stats_dir_missing) return while the library's thread still loads
the index.  That commit's binary never closed the index there and, on the MI355X, died in exit() with SIGABRT behind its own lines
instead of ending with its exit code; for them the fixture holds those lines and the exit code the `return` carries (see the
generator).  The program as it is now closes the index on every path, so here all four must end with that code and say nothing else."""
import json
import lzma
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
EXE = os.path.join(os.path.dirname(HERE), "kit4b_amd", "k4align")
SE, PE = ["-i", "../in/se.fa"], ["-i", "../in/pe_1.fa", "-u", "../in/pe_2.fa"]
PE_ARGS = ["-s2", "-U1", "-d200", "-D600"]

# name: (arguments behind `-I g1.sfx`, expected exit code)
CASES = {
    "se": (["-s2", "-o", "o.sam"] + SE, 0),
    "pe": (PE_ARGS + ["-o", "o.sam"] + PE, 0),
    "batches": (["-s2", "-b", "0.03", "-o", "o.sam"] + SE, 0),
    "slice": (["-s2", "-S", "0/2", "-o", "o.sam"] + SE, 0),
    "legacy": (["-s2", "-Z", "-o", "o.sam"] + SE, 0),
    "bam": (["-s2", "-t", "3", "-o", "o.bam"] + SE, 0),
    "pba": (["-s2", "-M3", "--experimentid", "e1", "--readsetid", "r1", "-o", "o.pba"] + SE, 0),
    "snp_markers_centroids": (["-s2", "-p5", "-K25", "-7", "cent.csv", "-o", "o.sam"] + SE, 0),
    "stats_siteprefs": (["-s2", "-O", "st.csv", "-8", "site.csv", "-o", "o.sam"] + SE, 0),
    "unaligned": (["-s2", "-j", "none.fa", "-o", "o.sam"] + SE, 0),
    # the early returns behind the opened index
    "refuse_r3_b": (["-s2", "-r3", "-b1", "-o", "o.sam"] + SE, 1),
    "refuse_a_S": (["-s2", "-a5", "-S", "0/2", "-o", "o.sam"] + SE, 1),
    "refuse_bam_b": (["-s2", "-b1", "-o", "o.bam"] + SE, 3),
    "missing_reads": (["-s2", "-o", "o.sam", "-i", "../in/se.fa", "-i", "nothing.fa"], 2),
    "missing_loci": (["-s2", "-5", "nothing.csv", "-o", "o.sam"] + SE, 2),
    "fewer_mates": (PE_ARGS + ["-Z", "-o", "o.sam", "-i", "../in/pe_1.fa", "-u", "../in/pe_2_short.fa"], 3),
    "out_dir_missing": (["-s2", "-O", "st.csv", "-8", "site.csv", "-o", "nowhere/o.sam"] + SE, 5),
    "stats_dir_missing": (["-s2", "-O", "nowhere/st.csv", "-8", "site.csv", "-o", "o.sam"] + SE, 5),
}


def make_inputs(base):
    """base/in: the reads of test_gpu_io.py's se_s2 and pe_u1 cases, and the mates' file with its last 10 records cut off"""
    os.makedirs(os.path.join(base, "in"))
    for src, dst in (("sam_se_s2.fa.xz", "se.fa"), ("sam_pe_u1_1.fa.xz", "pe_1.fa"), ("sam_pe_u1_2.fa.xz", "pe_2.fa")):
        with lzma.open(os.path.join(GOLDEN, src)) as f, open(os.path.join(base, "in", dst), "wb") as g:
            g.write(f.read())
    with open(os.path.join(base, "in", "pe_2.fa")) as f, open(os.path.join(base, "in", "pe_2_short.fa"), "w") as g:
        lines = f.read().splitlines(True)
        assert len(lines) > 40 and all(l.startswith(">") for l in lines[::2])  # FASTA, two lines per read
        g.writelines(lines[:-20])


def mask(line):
    line = re.sub(r"\d+\.\d\ds", "#s", line)
    return re.sub(r"\(\d+ bytes\) \+ \.bai", "(# bytes) + .bai", line)


def record(exe, base, name):
    """one case in base/<name> (make_inputs(base) has run): {"rc", "stderr": masked lines, "files": what the run left there}"""
    cwd = os.path.join(base, name)
    os.makedirs(cwd)
    env = {k: v for k, v in os.environ.items() if k not in ("K4_TRACE", "K4ALIGN_FAULT", "K4ALIGN_FAULT_PEERS")}
    p = subprocess.run([exe, "-I", os.path.join(GOLDEN, "g1.sfx")] + CASES[name][0], cwd=cwd, env=env, capture_output=True, text=True, timeout=120)
    files = sorted(os.path.relpath(os.path.join(d, f), cwd) for d, _, fs in os.walk(cwd) for f in fs)
    return {"rc": p.returncode, "stderr": [mask(l) for l in p.stderr.splitlines()], "files": files}


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    b = str(tmp_path_factory.mktemp("k4msg"))
    make_inputs(b)
    return b


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "k4align_messages.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(CASES)
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_k4align_says_and_leaves_what_it_did(base, recorded, name):
    want, got = recorded[name], record(EXE, base, name)
    print(json.dumps(got, indent=1))
    assert want["rc"] == CASES[name][1]  # the recorded run ended as the case is meant to
    assert got["rc"] == want["rc"]       # (a signal would be negative)
    assert got["stderr"] == want["stderr"]
    assert got["files"] == want["files"]
    if want["rc"] == 0:
        assert got["files"], name
        if name == "batches":
            m = re.search(r"\((\d+) batches\)", got["stderr"][-1])
            assert m and int(m.group(1)) >= 2
    else:  # nothing but the program's own words (no runtime abort text), and no output, side file or part left behind
        assert got["stderr"] and all(l.startswith("k4align: ") for l in got["stderr"]), got["stderr"]
        assert got["files"] == []
