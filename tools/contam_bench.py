"""Device time of kalign's contaminant flank trimming stage (`-H`, k4_contam_trims_dev) alone: n SE reads of 100 random bases against
64 seeded random contaminants of 33..60 bases in classes 1, 3, 5 and 7 (128 entries on each end of the read).
    python tools/contam_bench.py [n_reads=20000000] [out.json]
Two warm-up calls, then five timed ones (host clock around the call, which waits for its stream); beside it the prepare stage with the
trims (k4_prepare_reads_contam_dev) and without (k4_prepare_reads_trim_dev)."""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kit4b_amd as k4  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
L = 100
rng = np.random.default_rng(2024)
with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "c.fa")
    with open(p, "w") as f:
        for k in range(64):
            f.write(">c%d@1357\n%s\n" % (k, "".join("ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(33, 61))))))
    tbl = k4.load_contaminants(p)
ix = k4.SfxIndex.open(os.path.join(ROOT, "tests", "golden", "g1.sfx"))
dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(7)
reads = torch.randint(0, 4, (n * L + 64,), dtype=torch.uint8, device=dev, generator=g)
offs = torch.arange(n, dtype=torch.int64, device=dev) * L
lens = torch.full((n,), L, dtype=torch.int32, device=dev)
c5 = torch.empty(n + 1, dtype=torch.uint8, device=dev)
c3 = torch.empty(n + 1, dtype=torch.uint8, device=dev)
o2 = torch.empty(n + 1, dtype=torch.int64, device=dev)
l2 = torch.empty(n + 1, dtype=torch.int32, device=dev)
st = torch.cuda.current_stream().cuda_stream
lib = k4.lib()
tot = (C.c_uint64 * 4)()
u, o, ml = C.c_uint64(), C.c_uint64(), C.c_uint32()


def contam():
    ix._ck(lib.k4_contam_trims_dev(ix.h, tbl.ctypes.data, len(tbl), 0, n, 0, 0, 1, 0, reads.data_ptr(), offs.data_ptr(), lens.data_ptr(), None, None, 0,
                                   c5.data_ptr(), c3.data_ptr(), tot, st))


def prepare_with():
    ix._ck(lib.k4_prepare_reads_contam_dev(ix.h, 0, n, 50, 500, 0, 0, 1, 0, offs.data_ptr(), lens.data_ptr(), None, None, 0, c5.data_ptr(), c3.data_ptr(),
                                           o2.data_ptr(), l2.data_ptr(), C.byref(u), C.byref(o), C.byref(ml), tot, st))


def prepare_without():
    ix._ck(lib.k4_prepare_reads_trim_dev(ix.h, 0, n, 50, 500, 0, 0, 1, 0, offs.data_ptr(), lens.data_ptr(), None, None, 0, o2.data_ptr(), l2.data_ptr(),
                                         C.byref(u), C.byref(o), C.byref(ml), st))


def timed(fn):
    for _ in range(2):
        fn()
    ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


res = {"reads": n, "read_len": L, "contaminants": 64, "entries": int(len(tbl)), "device": torch.cuda.get_device_name(0), "reps": 5}
for name, fn in (("contam_trims_ms", contam), ("prepare_with_trims_ms", prepare_with), ("prepare_without_ms", prepare_without)):
    ms = timed(fn)
    res[name] = ms
    res[name + "_median"] = statistics.median(ms)
    print(name, " ".join("%.2f" % x for x in ms), flush=True)
res["reads_with_5p_trim"], res["reads_with_3p_trim"] = int((c5[:n] > 0).sum()), int((c3[:n] > 0).sum())
res["mean_trim_5p"] = float(c5[:n].float().mean())
res["contam_mreads_per_s"] = n / res["contam_trims_ms_median"] / 1e3
print(json.dumps(res))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
ix.close()
