"""bench.py's plain line and --dump-outputs on the CPU: bench.run() itself with the oracle engine (tests/bench_cpu_engine.py)
in one process.  A plain run leaves the --full legs out; the dumped files are the last timed step's records, the same on
every run with the same arguments."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "c1", "--chroms", "2", "--chrom-mbp", "0.03",
        "--reads", "400", "--max-subs", "2"]


@pytest.fixture
def bench(monkeypatch):
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "K4_BENCH_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)
    sys.path.insert(0, ROOT)
    import bench

    return bench


def _line(bench, capsys, argv):
    from bench_cpu_engine import OracleEngine

    eng = OracleEngine()
    bench.main(argv, engine=eng)
    out = capsys.readouterr().out
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1]), eng


def _oracle_results(bench):
    """the records of the workload's reads, recomputed here from bench.py's own generators and seeds"""
    import torch

    from oracle_bindings import Oracle

    a = bench.parse_args(ARGS)
    dev = torch.device("cpu")
    chrom_len = int(a.chrom_mbp * 1e6)
    seq = bench.make_genome(dev, a.chroms, chrom_len)
    reads, _ = bench.make_reads(seq, a.chroms, chrom_len, a.reads, a.read_len, bench.shard_seed(False, 0), dev)
    O = Oracle()
    s = seq.numpy()
    h = O.build(["chr%d" % (i + 1) for i in range(a.chroms)],
                [s[c * (chrom_len + 1): c * (chrom_len + 1) + chrom_len].copy() for c in range(a.chroms)], threads=2)
    O.set_max_iter(h, 5000)
    n, L = reads.shape
    r = O.kalign_batch(h, (reads.numpy().reshape(-1), np.arange(n, dtype=np.uint64) * L, np.full(n, L, dtype=np.uint32)),
                       max_subs=a.max_subs, threads=2)
    O.close(h)
    return r


def test_plain_line_leaves_the_full_legs_out(bench, capsys):
    d, eng = _line(bench, capsys, ARGS)
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and eng.n_steps == 4
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["unit"] == "Mreads/s" and d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] - 400 * 3 / (d["ms_per_step"] * 3 / 1e3) / 1e6) < 1e-9 * max(1.0, d["value"])
    assert d["cpu_baseline"] is None and d["e2e"] is None
    assert d["parity"]["truth_property_violations_rank0"] is None and d["parity"]["oracle_sample"] is None
    assert sum(v for v in d["parity"]["nar_histogram"].values()) == 400

    f, _ = _line(bench, capsys, ARGS + ["--full"])
    assert f["full"] is True and f["parity"]["truth_property_violations_rank0"] == 0
    assert f["parity"]["nar_histogram"] == d["parity"]["nar_histogram"]


def test_steps_must_be_positive(bench):
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_are_the_last_steps_records(bench, capsys, tmp_path):
    d, _ = _line(bench, capsys, ARGS + ["--dump-outputs", str(tmp_path / "a")])
    files = sorted(os.listdir(tmp_path / "a"))
    r = _oracle_results(bench)
    want = {"row", "nar_histogram"} | {"result_" + f for f in r["out"].dtype.names} | \
        {"hit_" + f for f in r["hits"].dtype.names}
    assert set(files) == {f + ".npy" for f in want}
    arr = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype == np.float64 for a in arr.values())
    assert sum(a.nbytes for a in arr.values()) <= 64 << 20
    assert np.array_equal(arr["row"], np.arange(400))  # fewer reads than the sample: every read
    for f in r["out"].dtype.names:
        assert np.array_equal(arr["result_" + f], r["out"][f].astype(np.float64)), f
    for f in r["hits"].dtype.names:
        assert np.array_equal(arr["hit_" + f], r["hits"][:, 0][f].astype(np.float64)), f
    nh = d["parity"]["nar_histogram"]
    assert arr["nar_histogram"].sum() == 400 and arr["nar_histogram"][1] == nh["AA"] and arr["nar_histogram"][3] == nh["NL"]


def test_dump_outputs_sample_is_fixed(bench, capsys, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ROWS", 100)
    _line(bench, capsys, ARGS + ["--dump-outputs", str(tmp_path / "a")])
    _line(bench, capsys, ARGS + ["--dump-outputs", str(tmp_path / "b")])
    rows = np.load(tmp_path / "a" / "row.npy")
    assert rows.size == 100 and np.all(np.diff(rows) > 0) and rows[-1] < 400
    r = _oracle_results(bench)
    assert np.array_equal(np.load(tmp_path / "a" / "result_nar.npy"), r["out"]["nar"][rows.astype(np.int64)].astype(np.float64))
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
