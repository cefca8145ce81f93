"""bench.py --dump-outputs on one GPU: a plain run (bench.main in this process, a small ragged frame) times exactly
--steps steps, leaves every --full leg out of its line and writes the last timed step's output buffer; a second run with
the same arguments writes the same bytes (seeded queries, seeded initial weights, deterministic training frames)."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4099  # not a multiple of the 32-query tile


def _run(capsys, out_dir):
    import bench

    bench.main(["--gpus", "1", "--steps", "3", "--warmup", "2", "--queries", str(N), "--settle-ms", "0",
                "--dump-outputs", str(out_dir)])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    return json.loads(line), np.load(out_dir / "radiance.npy")


def test_plain_run_dumps_the_last_step_and_repeats_bitwise(nrc, dev, capsys, tmp_path, monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NRC_BENCH_FULL"):
        monkeypatch.delenv(k, raising=False)
    r0, y0 = _run(capsys, tmp_path / "a")
    r1, y1 = _run(capsys, tmp_path / "b")
    assert r0["steps"] == 3 and r0["warmup"] == 2 and r0["full"] is False
    assert r0["ms_per_step"] > 0 and r0["unit"] == "M queries/s" and r0["higher_is_better"] is True
    assert r0["dtype"] == "f16" and r0["n_gpus"] == 1
    assert abs(r0["value"] - N / (r0["ms_per_step"] * 1e-3) / 1e6) <= 1e-6 * r0["value"]
    for k in ("train_step_ms", "train_step_graph_ms", "c4_n1", "c4_per_rank", "frame", "wide_c5", "hash",
              "tcnn_numerics", "cpu_baseline", "weak", "dp_exchange"):
        assert r0[k] is None, k
    assert r0["roofline"]["sustained"] is None
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["radiance.npy"]
    assert y0.dtype == np.float32 and y0.shape == (N, 3)
    assert np.isfinite(y0).all() and float(y0.std()) > 0.0
    np.testing.assert_array_equal(y0, y1)
