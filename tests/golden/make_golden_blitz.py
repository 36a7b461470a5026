"""Writes tests/golden/blitz_<group>.xz: the PSL body lines `ngskit4b blitz` itself writes for the crafted queries of
tests/blitz_craft.py against tests/golden/query_index.sfx.xz.  Needs the reference's sources; run from the repository root:
    python tests/golden/make_golden_blitz.py [reference root]
It builds oracle/_ref/ngskit4b (make -C oracle ngskit4b) and runs it once per group with one thread, so that the lines come in
query order, and with explicit -C -c -k -J -j -g -p -a -P -Q.  A fixture is the xz-compressed text of the PSL lines behind the
header (the header names the build and is left out).  Before a fixture is written the generator checks what the tests rely on:
the Python restatement (tests/blitz_ref.py) reproduces every line, reaches every branch counter blitz_craft.WANT lists for the
group, and meets no tie among the heads the reference kept.
"""
import lzma
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def restated_lines(index, names, lens_by_id, cases, lp, pp, counters):
    import blitz_ref
    import query_ref

    out = []
    for name, q in cases:
        nodes = query_ref.locate_query_seqs(index, q, *lp)
        paths, blocks = blitz_ref.blitz_paths(index, q, nodes, *pp, counters=counters)
        for p in paths:
            tid, nb, off = p[1], p[15], p[16]
            out.append(blitz_ref.psl_line(name, len(q), names[tid], lens_by_id[tid], p, blocks[off:off + nb]))
    return out


def main():
    import blitz_craft as bc
    import query_craft as qc
    import query_ref
    from oracle_bindings import Oracle

    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ngskit4b", "REF=" + ref_root], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")
    tnames, ts = qc.targets()
    oracle = Oracle()
    with tempfile.TemporaryDirectory() as tmp:
        sfx = os.path.join(tmp, "query_index.sfx")
        with lzma.open(os.path.join(HERE, "query_index.sfx.xz"), "rb") as f:
            open(sfx, "wb").write(f.read())
        h = oracle.open(sfx)
        index = query_ref.index_from_oracle(oracle, h)
        ents = oracle.entries(h)
        names = {e["entry_id"]: e["name"] for e in ents}
        lens_by_id = {e["entry_id"]: e["seq_len"] for e in ents}
        for group, (lp, pp, cases) in bc.groups().items():
            fa, psl = os.path.join(tmp, group + ".fa"), os.path.join(tmp, group + ".psl")
            with open(fa, "w") as f:
                for name, q in cases:
                    assert len(q) >= 100, name
                    f.write(">%s\n%s\n" % (name, "".join("ACGTN"[int(b)] for b in q)))
            core_len, core_delta, _, _, max_iter, match, mismatch = lp
            assert (match, mismatch) == (pp[0], pp[1]) and core_len > 18 and max_iter >= 100
            cmd = [exe, "blitz", "-T1", "-M0", "-i", fa, "-I", sfx, "-o", psl, "-F", os.path.join(tmp, group + ".log"),
                   "-C%d" % core_len, "-c%d" % core_delta, "-k%d" % max_iter, "-J%d" % match, "-j%d" % mismatch, "-g%d" % pp[2],
                   "-p%d" % pp[3], "-a%d" % pp[4], "-P%d" % pp[5], "-Q%d" % pp[6]]
            subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
            lines = open(psl).read().splitlines()
            body = [ln for ln in lines if ln.count("\t") == 20 and ln.split("\t")[0].isdigit()]
            counters = {}
            mine = restated_lines(index, names, lens_by_id, cases, lp, pp, counters)
            print(group, len(cases), "queries", len(body), "lines", sorted(counters.items()))
            assert mine == body, (group, [(a, b) for a, b in zip(mine, body) if a != b][:2], len(mine), len(body))
            missing = [k for k in bc.WANT[group] if not counters.get(k)]
            assert not missing, (group, missing)
            with lzma.open(os.path.join(HERE, "blitz_%s.xz" % group), "wb", preset=9) as f:
                f.write(("\n".join(body) + "\n").encode())
        oracle.close(h)


if __name__ == "__main__":
    main()
