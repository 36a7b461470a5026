"""tests/golden/k4align_messages.json: exit code, masked stderr lines and left files of every case of
tests/test_gpu_k4align_messages.py, from the `k4align` binary of the commit the refactored program has to equal (needs an MI355X).

    git checkout <that commit> -- kit4b_amd/csrc/k4align_main.cpp && make -C kit4b_amd/csrc ../k4align
    python tests/golden/make_golden_k4align_messages.py [path of that k4align]

The cases, the inputs and the masking are the test's own (CASES, make_inputs, record).  Data only.

Four cases are not run with that binary.  It returns from them while the library's thread is still loading the index, and on the
MI355X it then died inside exit() (SIGABRT, "malloc(): unaligned tcache chunk detected" behind its own lines) instead of ending with
its exit code -- the defect the owner of the run's handles removes.  What is written for them is what that binary says there before
it dies: the index line every run starts with (taken from the recorded "se" case) and the one line of the refusal (its format string
in that commit's source), with the exit code its `return` carries.

The one run of all 18 cases with that binary, record() as it is now, gave for these four:
    refuse_r3_b        rc -6, last line 'malloc(): unaligned tcache chunk detected'
    refuse_a_S         rc -6, last line 'malloc(): unaligned tcache chunk detected'
    stats_dir_missing  rc -6, last line 'malloc(): unaligned tcache chunk detected'
    missing_reads      rc -6, stderr ["k4align: index 'g1' 5 sequences, 125420 bp; minimum core size 8bp",
                                      "k4align: unable to open 'nothing.fa'", 'malloc(): unaligned tcache chunk detected']
and for the other fourteen what the fixture holds (refuse_bam_b, behind k4_open_wait, ended with its exit code 3).
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_k4align_messages as t  # noqa: E402

PARENT_DIES = {
    "refuse_r3_b": "k4align: -r3 / -r4 cluster over all reads of the run; they cannot be combined with -b or -S",
    "refuse_a_S": "k4align: -a / -A drop junctions no second read of the RUN supports; they cannot be combined with -b or -S",
    "missing_reads": "k4align: unable to open 'nothing.fa'",
    "stats_dir_missing": "k4align: unable to create/truncate output stats file 'nowhere/st.csv'",
}

if __name__ == "__main__":
    exe = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else t.EXE
    with tempfile.TemporaryDirectory() as base:
        t.make_inputs(base)
        out = {name: t.record(exe, base, name) for name in sorted(t.CASES) if name not in PARENT_DIES}
    for name, line in PARENT_DIES.items():
        out[name] = {"rc": t.CASES[name][1], "stderr": [out["se"]["stderr"][0], line], "files": []}
    out = {name: out[name] for name in sorted(out)}
    for name, r in out.items():
        print(name, r["rc"], r["files"], r["stderr"][-1:] if r["rc"] else "")
    for name, r in out.items():
        assert r["rc"] == t.CASES[name][1], (name, r)
    with open(os.path.join(HERE, "k4align_messages.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
