"""bench.py's plain and --full runs and --dump-outputs.

CPU: the dump's fixed sample (dump_outputs) on host tensors.  GPU: the real entry point on
cfg2 (128^3, 1e5 markers on a sphere), in this process: a plain run leaves the fields that take
runs of their own empty and times exactly --steps steps; --dump-outputs writes U and f of the
last timed step, the same from run to run; --full fills the other fields in."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

torch = pytest.importorskip("torch")

FULL_ONLY = ("roofline", "cpu_baseline", "breakdown_ms", "touched_points")


def test_dump_outputs_small_arrays_whole_large_ones_sampled(tmp_path):
    small = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    n = bench.DUMP_SAMPLE + 12345
    large = torch.arange(n, dtype=torch.float64)
    patches = [torch.full((2, 3), float(k)) for k in range(3)]  # a level's patch arrays, f32
    bench.dump_outputs(tmp_path / "a", {"U": small, "f0": large, "f1": patches})
    bench.dump_outputs(tmp_path / "b", {"f0": large.clone()}, "_rank1")
    U = np.load(tmp_path / "a" / "U.npy")
    assert U.dtype == np.float64 and np.array_equal(U, np.arange(12.0))
    f0 = np.load(tmp_path / "a" / "f0.npy")
    assert f0.dtype == np.float64 and f0.shape == (bench.DUMP_SAMPLE,)
    # the entries are their own indices: ascending, in range, spread over the whole array
    assert np.all(np.diff(f0) >= 0) and f0[0] >= 0 and f0[-1] < n
    assert f0[0] < 0.01 * n and f0[-1] > 0.99 * n
    # the sample depends on the size alone
    assert np.array_equal(f0, np.load(tmp_path / "b" / "f0_rank1.npy"))
    f1 = np.load(tmp_path / "a" / "f1.npy")
    assert f1.dtype == np.float64 and np.array_equal(f1, np.repeat([0.0, 1.0, 2.0], 6))


def _run(monkeypatch, capsys, *argv, config="cfg2"):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--config", config, *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "IBTK_BENCH_DEVICE", "IBTK_BENCH_BACKEND"):
        monkeypatch.delenv(k, raising=False)
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path, monkeypatch, capsys):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    recs = [_run(monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d))
            for d in ("a", "b")]
    for rec in recs:
        assert rec["metric"] == bench.METRIC and rec["unit"] == "marker-ops/s"
        assert rec["higher_is_better"] is True and rec["dtype"] == "f64"
        assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["full"] is False
        M = rec["config"]["markers"]
        assert rec["value"] == pytest.approx(2.0 * M / (rec["ms_per_step"] * 1e-3), rel=1e-9)
        assert all(rec[k] is None for k in FULL_ONLY)
        assert rec["config"]["bin"].startswith("3 re-binning(s)")  # the timed steps: --steps of them
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["U.npy", "f0.npy", "f1.npy", "f2.npy"]
    total = 0
    for name in ("U", "f0", "f1", "f2"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        total += a.nbytes
        assert a.dtype == np.float64 and a.ndim == 1 and a.shape == b.shape
        assert np.all(np.isfinite(a)) and np.abs(a).max() > 0
        # the same inputs and the same build: U bit for bit; f to the rounding of its sums,
        # should their order differ: a point of this sphere sums well under 1e3 terms no
        # larger than max|f|, so reordering moves it by less than 1e3 * 2^-53 * max|f| ~ 1e-13
        if name == "U":
            assert a.shape == (3 * M,) and np.array_equal(a, b)
        else:
            assert a.shape == (bench.DUMP_SAMPLE,)
            assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    assert total <= 64 << 20


@pytest.mark.gpu
def test_full_run_fills_the_other_fields(monkeypatch, capsys):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rec = _run(monkeypatch, capsys, "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert rec["full"] is True and rec["steps"] == 2
    assert rec["cpu_baseline"] is None  # --no-cpu-baseline
    assert set(rec["breakdown_ms"]) == {"bin", "interp", "zero", "spread"}
    assert len(rec["touched_points"]) == 3 and all(n > 0 for n in rec["touched_points"])
    assert rec["roofline"]["kernel_ms"]["spread"] > 0 and rec["roofline"]["lds_atomic"]["ds_add_wave_instr"] > 0


@pytest.mark.gpu
def test_level_run_dumps_each_component_over_all_patches(tmp_path, monkeypatch, capsys):
    """cfg5 (the 8^3-patch level): f<a> is component a's patch arrays joined in patch order,
    a sample of more entries than one patch holds, and not all zero (the markers' sheets cross
    the level); U is a sample of the 3e7 velocities."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rec = _run(monkeypatch, capsys, "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path), config="cfg5")
    assert rec["full"] is False and all(rec[k] is None for k in FULL_ONLY)
    assert rec["config"]["patches"] == [8, 8, 8]
    for name in ("U", "f0", "f1", "f2"):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float64 and a.shape == (bench.DUMP_SAMPLE,)
        assert np.all(np.isfinite(a)) and np.abs(a).max() > 0
