"""Golden outputs of kalign's priority regions (`-B <bed>`, `-V`; CKAligner::ProcCoredApprox's priority pass, ngskit4b/KAligner.cpp:9682-9770,
and CKAligner::FiltByPriorityRegions :4093-4155) from the REAL reference front end (`oracle/_ref/ngskit4b`), run with ONE thread.

    python tests/golden/make_golden_priority.py

Writes the genome's index as `ngskit4b index` built it (priority.sfx.xz), the genome itself (priority_genome.fa.xz), the read sets
(priority_<set>.fa.xz), the BED files (priority_<name>.bed) and per case of priority_cases.json what `ngskit4b kalign -B ... [-V]` wrote
(priority_<case>.sam.xz, `-M1` unless the case says otherwise) with its NAR histogram.  Data only.

The genome (seeded): D, a 2 kb segment in 2 identical copies (asm1, trusted1); T in 3 (asm1 twice, trusted2); M in 12 (rep); E in 2 copies
that differ in one base in 100, so that a read of 100 bases meets exactly one difference (asm2, trusted3); unique sequence around them and on `uniq`.
"""
import json
import lzma
import os
import random
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
NGS = os.path.join(ROOT, "oracle", "_ref", "ngskit4b")
RL = 100
# reads around the feature uniq:3000-3100 and around the feature of no bases uniq:5000-5000 (met by a span that covers 4999 and 5000)
EDGE_STARTS = (2899, 2900, 2901, 2950, 3000, 3050, 3098, 3099, 3100, 3101, 4899, 4900, 4901, 4950, 4999, 5000, 5001)


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def genome():
    rng = random.Random(20240611)
    D, T, M, E = rnd(rng, 2000), rnd(rng, 2000), rnd(rng, 2000), rnd(rng, 2000)
    E2 = list(E)
    for p in range(50, 2000, 100):
        E2[p] = "ACGT"[("ACGT".index(E2[p]) + 1 + rng.randrange(3)) % 4]
    E2 = "".join(E2)
    seqs, where = [], {}

    def build(name, parts):
        s = ""
        for key, p in parts:
            if key:
                where.setdefault(key, []).append((name, len(s)))
            s += p
        seqs.append((name, s))

    build("asm1", [("U1", rnd(rng, 3000)), ("D", D), (None, rnd(rng, 2000)), ("T", T), (None, "A" + rnd(rng, 999)), ("T", T), (None, "C" + rnd(rng, 499))])
    build("trusted1", [(None, rnd(rng, 500)), ("D", D), (None, rnd(rng, 500))])
    # the suffixes of the three copies of T sort by what follows them -- A, C, G -- and that is the order of a read's hits: the copy
    # that case b leaves uncovered (the second on asm1) lies BETWEEN the covered ones, which is where the reference's compaction shows
    build("trusted2", [(None, rnd(rng, 500)), ("T", T), (None, "G" + rnd(rng, 499))])
    build("rep", [x for _ in range(12) for x in (("M", M), (None, rnd(rng, 300)))])
    build("asm2", [(None, rnd(rng, 1000)), ("E", E), (None, rnd(rng, 1000))])
    build("trusted3", [(None, rnd(rng, 400)), ("E", E2), (None, rnd(rng, 400))])
    build("uniq", [("Q", rnd(rng, 8000))])
    return seqs, where


def sample(rng, seq, lo, hi, n, subs=0):
    """n reads of RL bases that start in [lo, hi - RL], either strand, `subs` substitutions each"""
    out = []
    for _ in range(n):
        p = rng.randrange(lo, hi - RL + 1)
        r = list(seq[p:p + RL])
        for q in rng.sample(range(5, RL - 5), subs):
            r[q] = "ACGT"[("ACGT".index(r[q]) + 1 + rng.randrange(3)) % 4]
        r = "".join(r)
        out.append(r if rng.random() < 0.5 else revcomp(r))
    return out


def read_sets(seqs, where):
    rng = random.Random(77)
    S = dict(seqs)
    at = lambda key, k=0: where[key][k]  # noqa: E731
    sets = {}
    n, o = at("D")
    sets["dup"] = sample(rng, S[n], o, o + 2000, 150) + sample(rng, S["asm1"], 0, 3000, 60) + sample(rng, S["uniq"], 0, 8000, 60) + \
        sample(rng, S["trusted1"], 0, 500, 20) + sample(rng, S[n], o + 200, o + 1800, 30, subs=1)
    n, o = at("T")
    sets["tri"] = sample(rng, S[n], o, o + 2000, 150) + sample(rng, S["asm1"], 0, 3000, 50) + sample(rng, S["trusted2"], 0, 500, 20)
    n, o = at("M")
    sets["rep"] = sample(rng, S[n], o, o + 2000, 150) + sample(rng, S["uniq"], 0, 8000, 50)
    (n1, o1), (n2, o2) = at("E", 0), at("E", 1)
    sets["subs"] = sample(rng, S[n1], o1, o1 + 2000, 120) + sample(rng, S[n2], o2, o2 + 2000, 120) + sample(rng, S[n1], o1, o1 + 2000, 40, subs=1) + \
        sample(rng, S[n2], o2, o2 + 2000, 40, subs=1) + sample(rng, S["uniq"], 0, 8000, 40)
    # span edges around the feature uniq:3000-3100 (BED end exclusive): reads that abut it, and that overlap it by exactly one base
    q = S["uniq"]
    edge = []
    for p in EDGE_STARTS:
        edge += [q[p:p + RL], revcomp(q[p:p + RL])]
    sets["edge"] = edge + sample(rng, q, 0, 8000, 180)
    # spliced reads: 60 bases, a 500 base intron, 40 bases; four reads per junction (an orphan junction is dropped), exons in uniq:1000-1400
    spl = []
    for j0 in (1100, 1180, 1260):
        for sh in (0, 3, 7, 12):
            a = j0 - 60 + sh
            r = q[a:j0] + q[j0 + 500:j0 + 500 + RL - (j0 - a)]
            spl += [r, revcomp(r)]
    sets["splice"] = spl + sample(rng, q, 0, 8000, 150) + sample(rng, S[at("D")[0]], at("D")[1], at("D")[1] + 2000, 60)
    # pairs: fragments of 250-450 bases from D on asm1 (with its flanks) and from unique sequence
    pe1, pe2 = [], []
    for name, lo, hi, cnt in (("asm1", 2600, 5400, 140), ("uniq", 0, 8000, 80), ("trusted1", 0, 3000, 40)):
        for _ in range(cnt):
            fl = rng.randrange(250, 451)
            p = rng.randrange(lo, hi - fl + 1)
            f = S[name][p:p + fl]
            a, b = f[:RL], revcomp(f[-RL:])
            if rng.random() < 0.5:
                a, b = b, a
            pe1.append(a)
            pe2.append(b)
    sets["pe_1"], sets["pe_2"] = pe1, pe2
    return sets


def beds(where):
    at = lambda key, k=0: where[key][k]  # noqa: E731
    d_asm, d_tr = at("D", 0), at("D", 1)
    t = where["T"]
    e_tr = at("E", 1)
    line = lambda nm, s, e, *rest: "\t".join([nm, str(s), str(e)] + list(rest)) + "\n"  # noqa: E731
    return {
        # the trusted copy of D, whole sequences for the unique reads
        "trusted": line("trusted1", 0, 3000, "t1", "0", "+") + line("trusted2", 0, 3000, "t2", "0", "-") + line("trusted3", 0, 2800, "t3", "0", "+"),
        # the copy of D on asm1 instead (the other one of the two: one of `trusted` / `asm` has the covered copy second in hit order)
        "asm": "track name=priority\n" + line(d_asm[0], d_asm[1], d_asm[1] + 2000) + line("uniq", 0, 8000),
        # two of the three copies of T: the one on trusted2 and the first on asm1; overlapping and abutting features
        "two_of_three": line(t[2][0], t[2][1], t[2][1] + 1200) + line(t[2][0], t[2][1] + 1000, t[2][1] + 2000) + line(t[0][0], t[0][1], t[0][1] + 1000) +
        line(t[0][0], t[0][1] + 1000, t[0][1] + 2000),
        "rep": line("rep", 0, 2000, "m1") + line("uniq", 0, 8000, "u"),
        "subs": line(e_tr[0], e_tr[1], e_tr[1] + 2000) + line("uniq", 0, 8000),
        "edge": "# one feature of 100 bases\n" + line("uniq", 3000, 3100, "edge", "0", ".") + line("UNIQ", 6000, 6001, "one_base") + line("uniq", 5000, 5000, "no_base"),
        # a name the index lacks; asm1, rep, asm2, uniq are not named
        "absent": line("nosuch", 0, 5000) + line("trusted1", 0, 1500) + line("chrZ", 10, 20) + line("uniq", 0, 4000),
        "splice": line("uniq", 1000, 1400, "exons") + line("trusted1", 0, 3000),
    }


# case: (read set(s), bed, kalign arguments)
CASES = {
    "a_nobed": (["dup"], None, ["-s2", "-M1"]),
    "a": (["dup"], "trusted", ["-s2", "-M1"]),
    "a_M0": (["dup"], "trusted", ["-s2"]),
    "b_r0": (["tri"], "two_of_three", ["-s2", "-M1", "-V"]),
    "b_r2_R5": (["tri"], "two_of_three", ["-s2", "-M1", "-V", "-r2", "-R5"]),
    "c": (["dup"], "asm", ["-s2", "-M1"]),
    "d": (["rep"], "rep", ["-s2", "-M1"]),
    "e_e1": (["subs"], "subs", ["-s3", "-e1", "-M1", "-V"]),
    "e_e2": (["subs"], "subs", ["-s3", "-e2", "-M1", "-V"]),
    "f": (["edge"], "edge", ["-s2", "-M1"]),
    "g": (["dup"], "absent", ["-s2", "-M1"]),
    "h_V": (["dup"], "trusted", ["-s2", "-M1", "-V"]),
    "i_u1": (["pe_1", "pe_2"], "trusted", ["-s2", "-M1", "-U1", "-d150", "-D600"]),
    "i_u3_V": (["pe_1", "pe_2"], "trusted", ["-s2", "-M1", "-U3", "-d150", "-D600", "-V"]),
    "j": (["splice"], "splice", ["-s5", "-a12", "-A3000", "-M1"]),
    "j_V": (["splice"], "splice", ["-s5", "-a12", "-A3000", "-M1", "-V"]),
}


def hist_of(log):
    hist = {}
    for line in open(log):
        m = re.search(r"\)\s+(\d+) \((\w\w)\) ", line)
        if m:
            hist[m.group(2)] = int(m.group(1))
    return hist


def write_xz(name, data):
    with lzma.open(os.path.join(HERE, name), "wb", preset=9) as g:
        g.write(data if isinstance(data, bytes) else data.encode())


def main():
    seqs, where = genome()
    sets = read_sets(seqs, where)
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "priority_genome.fa")
        with open(fa, "w") as f:
            for name, s in seqs:
                f.write(">%s\n" % name + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)))
        write_xz("priority_genome.fa.xz", open(fa).read())
        sfx = os.path.join(tmp, "priority.sfx")
        subprocess.run([NGS, "index", "-i", fa, "-o", sfx, "-r", "priority", "-T", "1", "-F", sfx + ".log"], check=True, capture_output=True, timeout=600)
        write_xz("priority.sfx.xz", open(sfx, "rb").read())
        files = {}
        for name, reads in sets.items():
            p = os.path.join(tmp, "priority_%s.fa" % name)
            tag = name[:-2] if name.startswith("pe_") else name
            with open(p, "w") as f:
                f.write("".join(">%s%04d\n%s\n" % (tag, k, r) for k, r in enumerate(reads)))
            write_xz("priority_%s.fa.xz" % name, open(p).read())
            files[name] = p
        for name, text in beds(where).items():
            with open(os.path.join(HERE, "priority_%s.bed" % name), "w", newline="") as f:
                f.write(text)
        meta, dropped = {}, {}
        for case, (rs, bed, args) in CASES.items():
            out = os.path.join(tmp, case + ".sam")
            cmd = [NGS, "kalign", "-I", sfx, "-o", out, "-T", "1", "-F", out + ".log"] + args
            if bed:
                cmd += ["-B", os.path.join(HERE, "priority_%s.bed" % bed)]
            for flag, r in zip(("-i", "-u"), rs):
                cmd += [flag, files[r]]
            try:
                p = subprocess.run(cmd, capture_output=True, timeout=600)
            except subprocess.TimeoutExpired:
                dropped[case] = "the reference did not end within 600 s"
                continue
            if p.returncode != 0:
                dropped[case] = "the reference ended with status %d" % p.returncode
                continue
            hist = hist_of(out + ".log")
            write_xz("priority_%s.sam.xz" % case, open(out, "rb").read())
            meta[case] = dict(reads=rs, bed=bed, args=args, nar=hist)
            print(case, {k: v for k, v in hist.items() if v})
        for case, why in dropped.items():
            print("DROPPED", case, why)
        with open(os.path.join(HERE, "priority_cases.json"), "w") as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(meta.items())) + "\n}\n")
        # ---- the cases exercise what they are there for
        m = meta
        assert m["a"]["nar"]["AA"] > m["a_nobed"]["nar"]["AA"] - m["a"]["nar"].get("PR", 0) and m["a_nobed"]["nar"]["ML"] >= 150
        assert m["h_V"]["nar"]["ML"] < m["a_nobed"]["nar"]["ML"] and m["h_V"]["nar"].get("PR", 0) == 0 and m["a"]["nar"]["PR"] > 0
        assert m["b_r0"]["nar"]["ML"] >= 150 and m["d"]["nar"]["ML"] >= 150
        same = lambda a, b: lzma.open(os.path.join(HERE, "priority_%s.sam.xz" % a)).read() == lzma.open(os.path.join(HERE, "priority_%s.sam.xz" % b)).read()  # noqa: E731
        # (e_e1 and e_e2 come out equal: AlignReads leaves at the first phase with a hit, whose mismatch limit hides the next best copy,
        # so LowMMCnt / NxtLowMMCnt never lie within -e2 of each other here, with or without the priority pass)
        assert not same("g", "a")
        assert m["g"]["nar"]["PR"] > 0 and m["f"]["nar"]["PR"] > 0 and m["f"]["nar"]["AA"] >= 10


if __name__ == "__main__":
    sys.exit(main())
