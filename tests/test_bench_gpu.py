"""bench.py's contract on the GPU: the JSON line's schema, and the N > 1 code path (process group on RCCL, exchange on a
side stream, two frames in flight) run with a ONE-rank group — the only way its RCCL calls can be exercised on a one-GPU
box (several ranks may not share a GPU under RCCL; the multi-rank logic itself is rehearsed with gloo, tests/test_sharded_gloo.py)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*args):
    env = dict(os.environ, MASTER_PORT="29541")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, "bench.py prints ONE JSON line"
    return json.loads(lines[0])


def test_bench_line_schema_and_one_rank_exchange_path():
    base = _bench("--full", "--size", "512", "--steps", "3", "--warmup", "1", "--cpu-sample", "48", "--extras", "0")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "rays_per_s", "frame_checksum"):
        assert k in base, k
    assert base["n_gpus"] == 1 and base["steps"] == 3 and base["warmup"] == 1 and base["dtype"] == "f64"
    assert base["higher_is_better"] is True and base["vs_baseline"] is None and base["data"] == "synthetic"
    assert "workload" in base["config"] and "model" not in base["config"]
    roof = base["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in roof, k
    assert roof["frac"] is None or 0.0 < roof["frac"] <= 1.0          # None: no profile of the current kernel sources
    assert roof["frac"] is not None or "stale_profile" in roof
    cpu = base["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["cores"] >= 1 and cpu["value"] > 0 and "sample" in cpu
    assert abs(base["value"] * base["ms_per_step"] * 1e-3 - base["step_attempts_per_pass"]) <= 1e-6 * base["step_attempts_per_pass"]
    # the N > 1 path on a one-rank RCCL group: same frame, bit for bit; status bytes gathered; two frames in flight
    ex = _bench("--full", "--size", "512", "--steps", "4", "--warmup", "1", "--exchange-at-n1")
    assert ex["frame_checksum"] == base["frame_checksum"]
    assert ex["exchange"] == "overlapped with the next pass" and ex["frames_in_flight"] == 2
    assert ex["gathered_status_not_event"] == 0 and ex["step_attempts_per_pass"] == base["step_attempts_per_pass"]
    assert ex["cpu_baseline"] is None                                  # the CPU leg is N = 1 only
    # what makes a multi-GPU line diagnosable: every rank's kernel times, rays, attempts and its exchange time
    assert len(ex["per_rank"]) == 1 and ex["per_rank"][0]["far_ms"] > 0 and ex["per_rank"][0]["exchange_ms"] > 0
    assert ex["per_rank"][0]["rays"] == 512 * 512 and ex["per_rank"][0]["step_attempts"] == base["step_attempts_per_pass"]
    assert ex["rank_imbalance"]["integrate_ms_max"] >= ex["rank_imbalance"]["integrate_ms_min"] > 0
    serial = _bench("--full", "--size", "512", "--steps", "2", "--warmup", "1", "--exchange-at-n1", "--no-overlap")
    assert serial["frame_checksum"] == base["frame_checksum"] and serial["exchange"] == "in turn"


def test_bench_plain_run_and_its_dumped_outputs(tmp_path):
    """A plain run (no --full) prints the headline line alone — no CPU baseline, roofline or checksum — with --steps timed steps;
    --dump-outputs writes the frame of the last timed step: the same bits as the frame --full checksums, in the run's dtype."""
    import numpy as np
    import torch
    plain = _bench("--size", "256", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 3 and plain["passes_in_process"] == 4 and plain["dtype"] == "f64"
    assert not {"roofline", "cpu_baseline", "frame_checksum", "entry_points", "variants"} & set(plain)
    assert abs(plain["value"] * plain["ms_per_step"] * 1e-3 - plain["step_attempts_per_pass"]) <= 1e-6 * plain["step_attempts_per_pass"]
    rgb = np.load(tmp_path / "plain" / "rgb.npy")
    assert rgb.dtype == np.float64 and rgb.shape == (3, 256 * 256)
    assert np.array_equal(np.load(tmp_path / "plain" / "pixel_index.npy"), np.arange(256 * 256.0))
    full = _bench("--full", "--size", "256", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--extras", "0",
                  "--dump-outputs", str(tmp_path / "full"))
    assert np.array_equal(np.load(tmp_path / "full" / "rgb.npy"), rgb)
    assert int(torch.from_numpy(rgb).view(torch.int64).sum().item()) == full["frame_checksum"]
    _bench("--size", "256", "--steps", "1", "--warmup", "1", "--dtype", "f32", "--dump-outputs", str(tmp_path / "f32"))
    assert np.load(tmp_path / "f32" / "rgb.npy").dtype == np.float32


def test_bench_counts_its_own_flops_and_bytes():
    """--live-counters 1: the roofline's executed flops per step attempt and the HBM bytes per ray are hardware-counted by the run
    itself (rocprofv3 --pmc passes of one frame in child processes) and agree with the committed profile of the same kernel
    sources — which is then the cross-check, not the source."""
    import shutil
    if not (shutil.which("rocprofv3") or os.path.exists("/opt/rocm/bin/rocprofv3")):
        pytest.skip("rocprofv3 is not on this box")
    d = _bench("--full", "--size", "1024", "--steps", "3", "--warmup", "1", "--cpu-sample", "0", "--extras", "0", "--live-counters", "1")
    roof = d["roofline"]
    assert roof["counters"] == "live", roof.get("live_counters_skipped")
    live = roof["live"]
    assert live["step_attempts_counted"] == d["step_attempts_per_pass"] and 600 < live["valu_per_wave_step"] < 1200
    assert 0.3 < roof["frac"] <= 1.0 and abs(roof["executed_flop_per_step_attempt"] - live["flop_per_step_attempt"]) < 1e-9
    assert 500 < live["hbm_bytes_per_ray"] < 1500 and roof["traffic"] > 0
    # … and the profiler's own average kernel durations (one more child run, --kernel-trace --stats) agree with the HIP-event times
    assert len(live["rocprof_kernel_trace"]) == 2 and all(v["calls"] == 4 for v in live["rocprof_kernel_trace"].values())
    assert 0.85 < roof["event_over_rocprof"] < 1.15
    if "profile_flop_per_step_attempt" in roof:      # same sources profiled at 4096²: small launches idle a few more lanes
        assert 0.9 < roof["live_over_profile"] < 1.15
    off = _bench("--full", "--size", "256", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--extras", "0")
    assert off["roofline"]["counters"] in ("profile", None) and "live" not in off["roofline"]


def test_bench_host_entry_points():
    """--entry host / pixels: the timed passes go through rtgr_trace_f64 / rtgr_trace_pixels_f64 (PCIe-inclusive)."""
    base = _bench("--full", "--size", "256", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--extras", "0")
    for entry in ("host", "pixels"):
        d = _bench("--full", "--size", "256", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--extras", "0", "--entry", entry)
        assert d["config"]["entry"] == entry and d["step_attempts_per_pass"] == base["step_attempts_per_pass"]
        assert d["value"] > 0 and d["roofline"]["launches"] >= 2


def test_bench_single_process_multi_device_entries():
    """--entry sharded (rtgr_trace_sharded_device_f64, frame gathered on device 0) and --entry pixels / host with
    --ctx-devices N (the drop-in host entries dealing rows to every device of the context): the delivered frame is the
    single-device frame bit for bit (frame_checksum) and the counters are the same job's.  One GPU: the context lists it N
    times, which the line says (ctx_note) — a rehearsal of the code path, not a scaling figure."""
    base = _bench("--full", "--size", "256", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--extras", "0")
    for args in (("--entry", "sharded", "--ctx-devices", "3"), ("--entry", "pixels", "--ctx-devices", "2"),
                 ("--entry", "host", "--ctx-devices", "4"), ("--entry", "host")):
        d = _bench("--full", "--size", "256", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--extras", "0", *args)
        assert d["frame_checksum"] == base["frame_checksum"], args
        assert d["step_attempts_per_pass"] == base["step_attempts_per_pass"] and d["n_gpus"] == 1
        if "--ctx-devices" in args:
            n = int(args[-1])
            assert d["ctx_devices"] == [0] * n and "rehearsal" in d["ctx_note"]
            assert len(d["per_device_kernel_ms"]) == n and all(v["far"] > 0 for v in d["per_device_kernel_ms"])
            assert d["roofline"]["achieved"] is None and "approximate" in d["roofline"]   # logical devices time-share one GPU: no roofline
        if args[1] == "sharded":   # peer-access table + the library's exchange timers, per device of the context
            assert [p["peer_access_with_device_0"] for p in d["peer_access"]] == [1, 1, 1]
            ex = d["exchange_per_device"]
            assert ex[0]["rows_out_ms"] == 0 and ex[0]["place_rows_ms"] > 0 and all(e["rows_out_ms"] > 0 and e["copies"] == 1 for e in ex[1:])
    for k in ("contract_8d_frac", "contract_8d_note"):
        assert k in base["roofline"]


def test_bench_two_rank_rehearsal_line_is_diagnosable():
    """The driver's N > 1 launch form with two gloo ranks sharing this one GPU (RCCL does not allow that; gloo stages the gather
    through the host): the line carries every rank's kernel times, rays, step attempts and exchange time, the imbalance summary,
    and the frame equals the N = 1 frame bit for bit.  A rehearsal of the code path — not a scaling figure."""
    base = _bench("--full", "--size", "256", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--extras", "0")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29547", os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--backend", "gloo",
                        "--size", "256", "--steps", "2", "--warmup", "1"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["world_size_checked"] == 2 and d["frame_checksum"] == base["frame_checksum"]
    assert d["step_attempts_per_pass"] == base["step_attempts_per_pass"] and d["gathered_status_not_event"] == 0
    pr = d["per_rank"]
    assert [p["rank"] for p in pr] == [0, 1] and sum(p["rays"] for p in pr) == 256 * 256
    assert sum(p["step_attempts"] for p in pr) == base["step_attempts_per_pass"]
    assert all(p["far_ms"] > 0 and p["near_ms"] > 0 and p["exchange_ms"] > 0 and p["wall_ms"] > 0 for p in pr)
    assert 1.0 <= d["rank_imbalance"]["max_over_mean"] < 4.0   # (two ranks time-share ONE GPU here: the bound only says the figure is sane)
    assert len(d["row_checksums_sha256"]) == 16 and "row_checksums" not in d          # the vector itself only on request


def test_bench_line_survives_a_wrong_row_and_names_rank_and_rows(tmp_path):
    """The failure path of the multi-GPU line (round-4 review: an assert BEFORE the print killed rank 0 without a line and left the other
    ranks in the closing barrier).  Rank 1 of a two-rank gloo rehearsal is made to deliver one wrong row (RTGR_BENCH_CORRUPT_RANK):
    the line must still appear — per_rank, exchange times and all —, say frame_checksum_ok false, name image row 3 (rank 1's local row 1
    of a cyclic deal) and rank 1, every rank must leave the barrier, and the run must fail with exit code 2 — no hang."""
    ref = tmp_path / "n1.json"
    base = _bench("--full", "--size", "256", "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--extras", "0", "--emit-row-checksums")
    assert len(base["row_checksums"]) == 256 and (sum(base["row_checksums"]) - base["frame_checksum"]) % 2 ** 64 == 0   # (int64 sums wrap)
    ref.write_text(json.dumps(base) + "\n")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29548", os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--backend", "gloo", "--size", "256",
           "--steps", "2", "--warmup", "1", "--checksum-reference", str(ref)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    good = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert good.returncode == 0, good.stderr[-3000:]
    d = json.loads([x for x in good.stdout.splitlines() if x.startswith("{")][0])
    assert d["frame_checksum_ok"] is True and d["frame_checksum_source"] == str(ref) and "frame_checksum_bad_rows" not in d
    bad = subprocess.run(cmd, capture_output=True, text=True, env=dict(env, RTGR_BENCH_CORRUPT_RANK="1"), timeout=600)
    assert bad.returncode != 0
    lines = [x for x in bad.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, bad.stderr[-3000:]
    d = json.loads(lines[0])
    assert d["frame_checksum_ok"] is False and d["frame_checksum"] != base["frame_checksum"]
    assert d["frame_checksum_bad_rows"]["count"] == 1 and d["frame_checksum_bad_rows"]["first"] == [3] and d["frame_checksum_bad_rows"]["ranks"] == [1]
    assert [p["rank"] for p in d["per_rank"]] == [0, 1] and all(p["exchange_ms"] > 0 for p in d["per_rank"])
    assert "exitcode  : 2" in bad.stderr or "exitcode: 2" in bad.stderr or "exit code 2" in bad.stderr.lower(), bad.stderr[-1500:]
    # the single-process forms attribute rows to CONTEXT DEVICES the same way (no corruption hook inside the library: the mapping only)
    sh = _bench("--full", "--size", "256", "--steps", "1", "--warmup", "1", "--cpu-sample", "0", "--extras", "0", "--entry", "sharded", "--ctx-devices", "2",
                "--checksum-reference", str(ref))
    assert sh["frame_checksum_ok"] is True and sh["row_checksums_sha256"] == base["row_checksums_sha256"]
