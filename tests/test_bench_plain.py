"""bench.py without --full: the timed steps and the result line only, and --dump-outputs (benchlib/dump.py), which writes what the last
timed step computed so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import dump as D


def test_dump_sample_is_fixed_ascending_and_bounded():
    a, b = D.sample_index(10_000_000), D.sample_index(10_000_000)
    assert len(a) == D.MAX_ROWS and (a == b).all()
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < 10_000_000
    assert (D.sample_index(1000) == np.arange(1000)).all()
    # index + score + 2-wide sink, float64: within the 64 MB a dump may take
    assert D.MAX_ROWS * 8 * 4 <= 64 << 20


def test_dump_writes_exact_float64_rows(tmp_path):
    n = 5000
    g = np.random.Generator(np.random.PCG64(7))
    score = torch.from_numpy(g.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32))
    sink = torch.from_numpy(g.integers(-(1 << 31), 1 << 31, (n, 2), dtype=np.int64).astype(np.int32))
    D.write_outputs(str(tmp_path), score, sink, max_rows=1024)
    idx, s, k = (np.load(tmp_path / (name + ".npy")) for name in ("index", "score", "sink"))
    assert idx.dtype == s.dtype == k.dtype == np.float64
    assert idx.shape == (1024,) and s.shape == (1024,) and k.shape == (1024, 2)
    i = idx.astype(np.int64)
    assert (i == D.sample_index(n, 1024)).all()
    assert (s == score.numpy()[i]).all() and (k == sink.numpy()[i]).all()


def test_bench_parser_keeps_the_extras_behind_full(monkeypatch):
    try:
        import bench
    except Exception as e:      # noqa: BLE001  (bench.py imports the library; on a box without the built .so this test has nothing to check)
        pytest.skip("bench.py not importable here: %r" % (e,))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


@pytest.mark.gpu
def test_plain_run_prints_one_line_and_dumps_the_last_step(tmp_path, cuda):
    """a plain run with a batch above the dump's row limit: one stdout line, no legs file, --steps timed steps; the dumped sample is the
    seeded one and its scores / sinks are the oracle's on the bench's own inputs"""
    import nvbio_amd as nvb  # noqa: F401
    from nvbio_amd import workloads as W
    from oracle import pyoracle as O
    import bench

    n = D.MAX_ROWS + 300_000
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--reads", str(n), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    h = json.loads(lines[0])
    assert h["metric"] == "aligned reads/s (100 bp, band=15)" and h["unit"] == "reads/s" and h["higher_is_better"] is True
    assert h["dtype"].startswith("int32") and h["steps"] == 5 and h["warmup"] == 2
    assert h["value"] > 0 and abs(h["value"] - n / (h["ms_per_step"] * 1e-3)) / h["value"] < 1e-6
    assert h["parity"] is None and h["cpu_baseline"] is None and "rank_roofline" not in h
    assert sorted(os.listdir(tmp_path)) == ["dump"]
    idx, score, sink = (np.load(out_dir / (name + ".npy")) for name in ("index", "score", "sink"))
    assert idx.dtype == score.dtype == sink.dtype == np.float64
    i = idx.astype(np.int64)
    assert (i == D.sample_index(n)).all() and score.shape == (D.MAX_ROWS,) and sink.shape == (D.MAX_ROWS, 2)
    # the bench's inputs, rebuilt here; a spread of the dumped rows against the oracle
    patterns, texts = W.make_sw_batch(n, bench.READ_LEN, bench.REF_LEN, seed=0x5EED0002, device=cuda)
    rows = torch.from_numpy(i[::250].copy()).to(cuda)
    sub_p = nvb.PackedStringSet(patterns.words, 4, True, patterns.begin[rows].contiguous(), None, bench.READ_LEN)
    sub_t = nvb.PackedStringSet(texts.words, 2, False, texts.begin[rows].contiguous(), None, bench.REF_LEN)
    es, ek = O.batch_banded_gotoh_score(bench.BAND, O.LOCAL, bench.SCHEME, O.StringSet.from_device(sub_p), O.StringSet.from_device(sub_t))
    assert (score[::250] == es).all()
    assert (sink[::250].astype(np.int64).astype(np.uint32) == ek).all()
