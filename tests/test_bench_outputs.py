"""bench.py --dump-outputs on the host: the file format, the 64 MiB budget and the fixed sample of utterances."""
import numpy as np

import bench


def _outputs(B, samples, rng):
    return {"o": rng.standard_normal((B, 1, samples)).astype(np.float32),
            "z": rng.standard_normal((B, 3, samples // 16)).astype(np.float32),
            "duration": rng.integers(0, 9, (B, 1, 7)),
            "f0": rng.standard_normal((B, 7))}


def test_small_outputs_are_written_whole(tmp_path):
    arr = _outputs(4, 4096, np.random.default_rng(0))
    info = bench.dump_outputs(str(tmp_path), arr)
    assert info["utterances"] == info["of"] == 4 and info["names"] == sorted(arr)
    for k, v in arr.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == (np.float32 if k in ("o", "z") else np.float64)
        assert np.array_equal(got, v)                  # integer durations exact in float64, f0 float64 as it came


def test_large_outputs_keep_one_seeded_sample_of_utterances_within_the_budget(tmp_path, monkeypatch):
    assert bench.DUMP_BUDGET_BYTES == 64 << 20
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    arr = _outputs(32, 16384, np.random.default_rng(1))
    info = bench.dump_outputs(str(tmp_path / "a"), arr)
    again = bench.dump_outputs(str(tmp_path / "b"), _outputs(32, 16384, np.random.default_rng(1)))
    assert info == dict(again, dir=info["dir"]) and 0 < info["utterances"] < 32
    total = sum((tmp_path / "a" / f"{k}.npy").stat().st_size - 128 for k in arr)     # (.npy header: 128 bytes)
    assert total == info["bytes"] <= 1 << 20
    rows = None
    for k, v in arr.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        assert np.array_equal(got, np.load(tmp_path / "b" / f"{k}.npy"))
        # every array keeps the same utterances, in index order
        idx = [int(np.flatnonzero([np.array_equal(g, x) for x in v.astype(got.dtype)])[0]) for g in got]
        assert idx == sorted(idx) and (rows is None or idx == rows)
        rows = idx
