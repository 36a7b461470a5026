"""What the REAL reference front end (`oracle/_ref/ngskit4b kalign -M1`) loads from the inputs of
tests/test_ingest_reference_cpu.py, for machines where it is not built.

    python tests/golden/make_golden_ingest.py

Writes tests/golden/ingest_reference.json.xz: sha256 of each case's input text -> the sorted (name, sequence) records of the
reference's SAM, or null where it refused the file.  Data only."""
import hashlib
import json
import lzma
import os
import pathlib
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_ingest_reference_cpu as t  # noqa: E402

assert os.path.exists(t.NGS), "needs oracle/_ref/ngskit4b (make -C oracle ngskit4b)"
out = {}
for case in t.CASES + ["sloughed"]:
    text, ext = t.case_input(case)
    with tempfile.TemporaryDirectory() as d:
        recs = t.reference_dump(pathlib.Path(d), HERE, text, ext)
    out[hashlib.sha256(text).hexdigest()] = None if recs is None else [(n.decode("latin-1"), q.decode("latin-1")) for n, q in recs]
    print(case, "refused" if recs is None else "%d records" % len(recs))
with lzma.open(os.path.join(HERE, t.GOLDEN), "wt", preset=9) as f:
    json.dump(out, f, sort_keys=True)
