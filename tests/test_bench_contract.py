"""Driver-contract guard for bench.py (CPU-only): the flags the driver
passes must parse, and the JSON the driver parses must name the
BASELINE.json metric/config.  Protects the contract from refactors
without needing a GPU."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_driver_flags_parse():
    """`bench.py --gpus N --steps K --warmup W` plus every documented
    knob must parse (the driver and torchrun pass exactly these)."""
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--help"],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--batch", "--subs",
                 "--dhcp-frac", "--stride", "--no-latency",
                 "--no-host-io", "--no-sort", "--no-overlap",
                 "--steer-all", "--svc-cus", "--full", "--dump-outputs"):
        assert flag in r.stdout, flag


def test_secondary_phases_only_under_full():
    """A plain run measures the headline alone: every secondary phase
    (launched-batch latency, downlink, persistent service, host-io)
    sits behind --full."""
    src = open(os.path.join(REPO, "bench.py")).read()
    tail = src[src.index("elapsed = time.perf_counter() - t_start"):]
    for call in ("launcher.dhcp_fastpath(", "launcher.downlink(",
                 "service_latency(launcher", "host_io_phase("):
        i = tail.index(call)
        guard = tail.rindex("\n    if ", 0, i)
        assert tail[guard:].lstrip().startswith("if args.full and "), call


def test_dump_outputs_files(tmp_path):
    """--dump-outputs writes verdict/out_len for the whole batch and a
    fixed seeded sample of packet rows, as float .npy, identically on
    every call."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    n, stride = 20000, 128
    g = torch.Generator().manual_seed(5)
    d = torch.randint(0, 256, (n, stride), dtype=torch.uint8, generator=g)
    v = torch.randint(0, 4, (n,), dtype=torch.uint8, generator=g)
    ol = torch.randint(-1, 500, (n,), dtype=torch.int16, generator=g)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, (d, v, ol), 0, 1)
    bench.dump_outputs(b, (d, v, ol), 0, 1)
    names = sorted(os.listdir(a))
    assert names == ["out_len.npy", "packet_rows.npy", "packets.npy",
                     "verdict.npy"]
    total = 0
    for name in names:
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        assert x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, y)
        total += x.nbytes
    assert total <= 64 << 20
    rows = np.load(os.path.join(a, "packet_rows.npy")).astype(np.int64)
    assert len(rows) == bench.DUMP_PACKET_ROWS and len(set(rows)) == len(rows)
    assert np.array_equal(np.load(os.path.join(a, "verdict.npy")),
                          v.numpy().astype(np.float32))
    assert np.array_equal(np.load(os.path.join(a, "out_len.npy")),
                          ol.numpy().astype(np.float32))
    assert np.array_equal(np.load(os.path.join(a, "packets.npy")),
                          d.numpy()[rows].astype(np.float32))


def test_output_schema_names_baseline_metric():
    """The result dict construction in bench.main must carry every
    driver-required key and echo the BASELINE benchmark name."""
    src = open(os.path.join(REPO, "bench.py")).read()
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"steps"',
                '"warmup"', '"ms_per_step"', '"higher_is_better"',
                '"scaling"', '"vs_baseline"', '"dtype"', '"data"',
                '"config"', '"global_batch"', '"seq_len"',
                '"parallelism"'):
        assert key in src, key
    with open(os.path.join(REPO, "BASELINE.json")) as f:
        base = json.load(f)
    # the benchmark string printed in config must be the BASELINE
    # metric (bench wraps it across source lines; compare collapsed)
    collapsed = " ".join(src.replace('"', " ").split())
    assert " ".join(base["metric"].split()) in collapsed
    # weak scaling + aggregate-value semantics stay declared
    assert '"scaling": "weak"' in src or "'scaling': 'weak'" in src or \
        '"weak"' in src
    assert "world * args.batch * args.steps" in src  # whole-job aggregate
    assert "ReduceOp.MAX" in src                     # MAX over ranks


def test_timed_region_is_barriered_and_synced():
    """Exactly K steps between barrier+synchronize pairs."""
    src = open(os.path.join(REPO, "bench.py")).read()
    i_start = src.index("t_start = time.perf_counter()")
    i_end = src.index("elapsed = time.perf_counter() - t_start")
    timed = src[i_start:i_end]
    assert "for k in range(args.steps):" in timed
    assert "torch.cuda.synchronize()" in timed
    before = src[:i_start]
    assert before.rstrip().endswith("torch.cuda.synchronize()")
