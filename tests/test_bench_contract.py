"""The driver contract: bench.py emits one valid JSON line (CPU mode)."""
import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_bench_cpu_smoke():
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--cpu", "--smoke", "--no-rtt",
         "--size-mb", "0.25", "--keys-per-server", "4"],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    j = json.loads(lines[0])
    assert j["unit"] == "GB/s"
    assert j["value"] > 0
    assert j["n_gpus"] == 1
    assert j["higher_is_better"] is True
    assert j["data"] == "synthetic"
    # the metric string is the driver's join key against BASELINE.json
    baseline = json.loads((REPO / "BASELINE.json").read_text())
    assert j["metric"] == baseline["metric"], (j["metric"], baseline["metric"])


def _run_bench(*flags):
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--cpu", "--size-mb", "1",
         "--keys-per-server", "1", *flags],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last step's pulled buffers as float32
    .npy files, identical from run to run; --steps is the timed count."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        j = _run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / name))
        assert j["steps"] == 3 and j["warmup"] == 1
        assert j["ms_per_step"] > 0
        files = sorted(p.name for p in (tmp_path / name).iterdir())
        assert files == [f"pull_key{k:04d}.npy" for k in range(8)], files
        dumps.append({f: np.load(tmp_path / name / f) for f in files})
    for f, a in dumps[0].items():
        assert a.dtype == np.float32 and a.shape == (1 << 18,)
        assert np.isfinite(a).all() and a.std() > 0.5  # the N(0,1) payload, not zeros
        assert np.array_equal(a, dumps[1][f]), f
    # every key carries its own payload
    assert not np.array_equal(dumps[0]["pull_key0000.npy"], dumps[0]["pull_key0001.npy"])


def test_dump_outputs_samples_large_buffers(tmp_path):
    """Buffers over the 64 MB budget are cut to a seeded sample: sorted
    distinct elements of the buffer, the same ones on every call."""
    import numpy as np

    sys.path.insert(0, str(REPO))
    import bench

    class FakeBuf:
        def __init__(self, arr):
            self.arr = arr

        def to_numpy_f32(self):
            return self.arr.copy()

    n = 4 << 20  # 4 x 16 MiB > budget; values stay exact in float32
    bufs = [(f"b{i}", FakeBuf(np.arange(n, dtype=np.float32) + i * n)) for i in range(4)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bufs, bf16=False)
    total = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    assert 32 << 20 < total <= 64 * 10**6
    for i in range(4):
        a = np.load(tmp_path / "a" / f"b{i}.npy")
        assert a.dtype == np.float32
        assert np.all(np.diff(a) > 0) and a[0] >= i * n and a[-1] < (i + 1) * n
        assert np.array_equal(a, np.load(tmp_path / "b" / f"b{i}.npy"))
    # bf16 payloads widen exactly: 0x3F80 is 1.0, 0xC000 is -2.0
    raw = np.array([0x3F80, 0xC000], dtype=np.uint16).view(np.float32)
    bench.dump_outputs(str(tmp_path / "h"), [("h", FakeBuf(raw))], bf16=True)
    assert np.load(tmp_path / "h" / "h.npy").tolist() == [1.0, -2.0]


def test_bench_full_adds_rtt():
    """The round-trip latency measurement runs only under --full."""
    plain = _run_bench("--steps", "2", "--warmup", "1")
    assert plain["config"]["p50_rtt_us"] == {}
    full = _run_bench("--steps", "2", "--warmup", "1", "--full", "--rtt-iters", "5")
    assert full["config"]["p50_rtt_us"]["1mb"] > 0
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[key] == full[key]


def test_rn50_buckets_shape():
    from ps_lite_amd.models import resnet50_grad_buckets, resnet50_param_sizes

    total = sum(resnet50_param_sizes())
    assert abs(total - 25_557_032) < 60_000, total  # ~25.5M params
    buckets = resnet50_grad_buckets()
    assert sum(buckets) == total * 4
    assert max(buckets) <= 4 << 20


def test_bench_cpu_rn50_contract():
    """`bench.py --cpu --mode rn50` runs BytePS reduce rounds on the CPU
    reduce handle and emits the JSON contract line."""
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--cpu", "--mode", "rn50",
         "--smoke", "--no-rtt"],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    j = json.loads(lines[0])
    assert j["config"]["mode"] == "rn50-cpu"
    assert j["value"] > 0
