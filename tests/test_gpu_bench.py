"""bench.py at one rank on the GPU, shortened.  A plain run times its K steps only and can dump the
last step's outputs.  With --full (the driver's N = 1 line before the option existed): the timed loop issues the K
steps eagerly (the default since round 6) or replays them from one HIP graph (RLE_BENCH_GRAPH=1), the
round trip is verified, the other issue form is timed beside it (value_eager and value_graph both
in the line, `value` the faster of them), and the per-kernel split of the timed loop's GPU time stays below the step time
(VERDICT r3 item 5)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("graph", ["1", "0"])
def test_bench_one_rank(graph):
    env = dict(os.environ, RLE_BENCH_GRAPH=graph)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "8", "--warmup", "3", "--full",
                        "--no-cpu", "--no-north-star", "--no-concurrent"], env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["verified_bit_exact_roundtrip"] is True
    assert out["value"] == max(out["value_eager"], out["value_graph"]), out
    assert out["kernels"]["roundtrip"]["us"] <= out["ms_per_step"] * 1000 * 1.02, (out["kernels"], out["ms_per_step"])
    assert out["value_eager"] > 0 and out["value_graph"] > 0, out
    assert ("graph" in out["issue"].split("(")[0]) is (out["value_graph"] > out["value_eager"]), out["issue"]


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    """A plain run times its steps and nothing else (what --full adds is absent from the line), and
    --dump-outputs writes the last timed step's results: every compressed size and status, and the
    seeded samples of the compressed and decoded bytes, equal to the oracle's at the same positions."""
    import numpy as np

    preinit = os.environ.get("RLE_MI355X_PREINIT")
    import bench   # (sets a default for its own process; later tests' child processes must not inherit it)
    if preinit is None:
        os.environ.pop("RLE_MI355X_PREINIT", None)
    import rle_mi355x as R
    import rle_oracle as O

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RLE_BENCH_GRAPH", "RLE_BENCH_PAD"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 7 and out["warmup"] == 2 and out["full"] is False
    assert out["unit"] == "GiB/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    for k in ("kernels", "roofline", "cpu_baseline", "north_star_dec64k", "concurrent_streams", "value_graph",
              "verified_bit_exact_roundtrip"):
        assert out[k] is None, k
    # value and ms_per_step describe the same timed steps (both rounded in the line: 3 and 4 decimals)
    u = out["config"]["u_bytes_per_gpu"]
    assert out["value"] == pytest.approx(u / (out["ms_per_step"] * 1e-3) / 2**30, rel=2e-2)
    assert out["value"] == out["value_eager"] and out["outputs_dumped"] == ["clen", "decoded", "encoded", "status"]

    got = {n: np.load(tmp_path / (n + ".npy")) for n in out["outputs_dumped"]}
    assert got["clen"].dtype == got["status"].dtype == np.float64
    assert got["encoded"].dtype == got["decoded"].dtype == np.float32
    assert sum((tmp_path / (n + ".npy")).stat().st_size for n in got) <= 64_000_000
    wl = bench.WORKLOADS["cfg1"]
    n, U = wl["n"], wl["size"]
    xs = [O.gen(wl["kinds"][i % len(wl["kinds"])], i, U) for i in range(n)]
    ys = [O.encode(x) for x in xs]
    assert np.array_equal(got["clen"], np.array([len(y) for y in ys], np.float64))
    assert int(got["clen"].sum()) == out["config"]["c_bytes_rank0"]
    assert not got["status"].any()
    coffs, ctotal = R.compressed_slots([U] * n)
    arena = np.zeros(ctotal, np.uint8)
    for y, o in zip(ys, coffs):
        arena[o:o + len(y)] = np.frombuffer(y, np.uint8)
    rng = np.random.default_rng(bench.DUMP_SEED)   # the samples' order: compressed, then decoded
    ci = bench._sample(ctotal, bench.DUMP_ENC_VALUES, rng, "cpu").numpy()
    di = bench._sample(n * U, bench.DUMP_DEC_VALUES, rng, "cpu").numpy()
    assert len(ci) < ctotal and len(di) < n * U   # (this workload is sampled, not dumped whole)
    assert np.array_equal(got["encoded"], arena[ci].astype(np.float32))
    assert np.array_equal(got["decoded"], np.frombuffer(b"".join(xs), np.uint8)[di].astype(np.float32))
