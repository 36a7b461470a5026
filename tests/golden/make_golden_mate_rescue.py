"""What the REAL reference (`oracle/_ref/libk4ref.so`, CSfxArray::AlignPairedRead with MinChimericLen) returned for the calls of
tests/test_oracle_ext.py::test_chimeric_mate_rescue_vs_live_reference, for machines where it is not built.

    python tests/golden/make_golden_mate_rescue.py

Writes tests/golden/mate_rescue_x_reference.json.xz: "<window>_<seed>" -> per call [sha256 of the arguments, rslt, hit record
bytes (hex)].  Data only; the index is tests/golden/g1.sfx."""
import json
import lzma
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import synth  # noqa: E402
import test_oracle_ext as t  # noqa: E402
from oracle_bindings import Ref, ref_available  # noqa: E402

assert ref_available(), "needs oracle/_ref/libk4ref.so (make -C oracle ref)"
names, chroms = synth.golden_genome()
R = Ref()
hr = R.open(os.path.join(HERE, "g1.sfx"))
out = {}
for window, seed in ((400, 1), (900, 2), (1500, 3), (6000, 4)):
    calls = []
    for _, args in t.rescue_calls(chroms, window, seed):
        r, h = R.align_paired_read_x(hr, *args)
        calls.append([t.rescue_args_digest(args), int(r), h.tobytes().hex()])
    out["%d_%d" % (window, seed)] = calls
    print(window, seed, len(calls), "calls")
R.close(hr)
with lzma.open(os.path.join(HERE, t.RESCUE_GOLDEN), "wt", preset=9) as f:
    json.dump(out, f, sort_keys=True)
