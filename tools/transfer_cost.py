#!/usr/bin/env python3
"""What volume emission costs (include/rtgr.h "volume emission"; profiles/transfer/README.md holds the figures).

    python tools/transfer_cost.py [--n 1024] [--rounds 3] [--json FILE]

The Kerr a = 0.9 scene of examples/hot_flow.py at n x n, Float64, host entry points (so every figure holds the copies of the frame to
the host: both sides of a ratio pay them).  Interleaved rounds of
  * the observer frame (rtgr_trace_observer_f64) and the transfer frame of the same scene (rtgr_trace_transfer_f64);
  * the observer frame through the simple tile kernel (option tile = 1): one lane per ray, the whole adaptive loop inline — the kernel
    whose structure the transfer kernel has, and so its yardstick.
Reported: the median times, the transfer pass alone (transfer frame - observer frame), its step attempts per second beside the tile
kernel's, and the multiple.  The transfer kernel integrates 10 components and evaluates a dual-number metric for the orbit's rate at
every stage: a multiple of the tile kernel per step is expected, and is reported as it is."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

rt = load_package()
abi = rt._abi


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    n, rounds, out = arg("--n", 1024), arg("--rounds", 3), arg("--json", "")
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    metric = rt.KerrSchild(1.0, 0.9)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -60.0)]
    inc = np.radians(60.0)
    pos = (0.0, 40 * np.sin(inc), 0.0, 40 * np.cos(inc))
    obs = rt.Observer(pos, (0, -pos[1], -pos[2], -pos[3]), (0, 0, 0, 1), 0.6, 0.45, max_batch_rays=n * n)
    opt = rt.solver_defaults(max_steps=4000, lambda1=400.0)
    flow = rt.Flow(j0=0.027, kappa=0.0, r0=4.0, alpha=1.5, H=0.4, s=0.5, r_stop=1.75)

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    runs = {"observer": lambda: rt.trace_observer(metric, objs, obs, n, n, opt=opt),
            "transfer": lambda: rt.trace_transfer(metric, objs, obs, n, n, flow, opt=opt)}

    def tile():
        with abi.options(lib, tile=1):
            return rt.trace_observer(metric, objs, obs, n, n, opt=opt)
    runs["tile"] = tile
    for fn in runs.values():   # warm-up: workspace, scratch, staging
        fn()
    times, last = {k: [] for k in runs}, {}
    for _ in range(rounds):
        for k, fn in runs.items():
            t, last[k] = timed(fn)
            times[k].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    tc, oc, kc = last["transfer"]["transfer_counters"], last["observer"]["counters"], last["tile"]["counters"]
    t_steps, k_steps = tc["accepted"] + tc["rejected"], kc["accepted"] + kc["rejected"]
    t_pass = med["transfer"] - med["observer"]
    res = dict(n=n, rounds=rounds, seconds=times, median=med, transfer_pass_s=t_pass, transfer_attempts=t_steps, trace_attempts=oc["accepted"] + oc["rejected"],
               tile_attempts=k_steps, transfer_attempts_per_s=t_steps / t_pass, tile_attempts_per_s=k_steps / med["tile"],
               frame_ratio=med["transfer"] / med["observer"])
    res["step_cost_multiple"] = res["tile_attempts_per_s"] / res["transfer_attempts_per_s"]
    print(json.dumps(res))
    if out:
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
