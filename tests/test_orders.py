"""Higher-order disk images (include/rtgr.h "higher-order disk images"): rays followed through the emitting disk,
order by order.  CPU: the declarations, the struct, the construction itself on the oracle (every crossing leg ends as an event on the
inflated disk at distance eta from the disk), the stored truth chains.  GPU: the call against the same chain spelled out through the
public API, bit for bit; order 0 and T = 0 against the emitted observer frame; true geodesics; where the rings lie; the per-order planes
fed to the stages; the refusals."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import truth
from conftest import ROOT
from scenes import rt
from test_observer import np_frame, np_rays, oracle_metric

abi = rt._abi
ORD_EXPORTS = ("rtgr_trace_orders_device_f64", "rtgr_trace_orders_device_f32", "rtgr_trace_orders_f64", "rtgr_trace_orders_f32")
DISK = (0.05, 3.0, 12.0)       # h, r_in, r_out
ETA = 0.025                    # the default margin: h / 2
DISK_OBJECT = 2                # its 1-based place in the list
T_FRAME = 30000.0
SIZES = ((64, 48), (37, 19))
GOLDEN = os.path.join(ROOT, "tests", "golden", "truth_orders.npz")
# the pixels of the 64 x 48 Kerr frame whose truth chains are stored (tests/golden/make_orders_truth.py): order 1 and order 2, spread in rho
TRUTH_BOUND = 3e-11            # the project's bound on a traced end state against a true geodesic


# ---- the two scenes of the issue ---------------------------------------------------------------------------------------------------------
def kerr_scene(a=0.9, sky=-30.0):
    return rt.KerrSchild(1.0, a), [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), sky), rt.Disk(*DISK)]


def plus_objs(eta=ETA):
    """the one object of S+: the inflated disk"""
    return [rt.Disk(DISK[0] + eta, DISK[1] - eta, DISK[2] + eta)]


def observer(max_batch_rays=0):
    """static, at (0, 0, -18, 9), looking at the origin.  The field of view holds the whole disk and little else, so that 64 x 48 pixels
    resolve the rings: an equirectangular frame (uniform in angle: finer at the centre, where the rings are, than a perspective frame of
    the same width) of 1.25 x 0.98 rad — the disk's image, lensed far side included, spans 0.61 rad to either side and 0.47 rad up and
    down, and stays off the frame's border rows and columns (test_oracle_chain_crossing_legs_end_on_the_inflated_disk holds that)."""
    return rt.Observer((0, 0, -18, 9), (0, 0, 18, -9), (0, 0, 0, 1), 1.25, 0.98, projection="equirect", max_batch_rays=max_batch_rays)


def solver(dtype=np.float64, lambda1=200.0):
    return rt.solver_defaults(dtype, max_steps=4000, lambda1=lambda1)


def emission():
    return rt.DiskEmission(DISK_OBJECT, T_FRAME)


def cpu_states(metric, ob, ni, nj):
    """the observer's ray states from the header's rule in numpy (tests/test_observer.py holds the device against it)"""
    g, dg = oracle_metric(metric, ob.pos[:])
    fr = np_frame(g, dg, ob)
    assert fr["valid"]
    return np_rays(g, fr["frame"], ob, ni, nj)


def strip_states(metric, nrays=256):
    """the Schwarzschild strip: parallel rays from (0, x, 0, -50) along +z, x = linspace(4.9, 6.2); past-directed null states, and the
    impact parameter b = |x cross p| / |p_t| of each from the covariant momentum"""
    sc = rt.make_scene(metric, [], units=False)
    xs = np.linspace(4.9, 6.2, nrays)
    s = np.zeros((nrays, 8))
    b = np.zeros(nrays)
    for q, x in enumerate(xs):
        pos = np.array([0.0, x, 0.0, -50.0])
        g = ol.metric_plain(sc, pos[None, :])[0]
        n = np.array([0.0, 0.0, 0.0, 1.0])
        t = np.linalg.solve(g, np.array([1.0, 0, 0, 0]))
        u = (t / np.sqrt(-t @ g @ t) + n / np.sqrt(n @ g @ n)) / np.sqrt(2.0)
        s[q] = np.concatenate([pos, u])
        p = g @ u
        b[q] = np.linalg.norm(np.cross(pos[1:], p[1:])) / abs(p[0])
    return s, b


# ---- the chain, leg by leg, over any tracer ----------------------------------------------------------------------------------------------
def chain(leg, s0, objs, N, eta=ETA):
    """leg(objs, states) -> dict(state_end, hit, status, ...).  -> (leg 0, [per order k = 1..: dict(idx: the pixels of the continuation
    leg, cross: the crossing leg of the rays that went into it (with `go`: which of them left by an event on object 1), cont: the
    continuation leg)])"""
    leg0 = leg(objs, s0)
    idx = np.flatnonzero(leg0["hit"] == DISK_OBJECT)
    se = leg0["state_end"][idx]
    orders = []
    for _ in range(N):
        if idx.size == 0:
            break
        cross = leg(plus_objs(eta), se)
        go = (cross["status"] == 0) & (cross["hit"] == 1)
        cross["go"], cross["idx"] = go, idx
        idx = idx[go]
        if idx.size == 0:
            orders.append(dict(idx=idx, cross=cross, cont=None))
            break
        cont = leg(objs, cross["state_end"][go])
        orders.append(dict(idx=idx, cross=cross, cont=cont))
        on = cont["hit"] == DISK_OBJECT
        idx, se = idx[on], cont["state_end"][on]
    return leg0, orders


def oracle_leg(metric, opt):
    def leg(objs, states):
        sc = rt.make_scene(metric, objs, units=False)
        return ol.trace(sc, opt, len(states), 1, state0=states)
    return leg


def truth_leg(metric, opt):
    def leg(objs, states):
        sc = rt.make_scene(metric, objs, units=False)
        rows = [truth.trace_ray(sc, opt, s, max_step=0.05) for s in states]
        # (an event of the truth tracer: the ray ended on an object before lambda1)
        return dict(state_end=np.array([r["state_end"] for r in rows]).reshape(-1, 8), hit=np.array([r["hit"] for r in rows], np.uint32),
                    status=np.array([0 if r["lambda_end"] < opt.lambda1 else 1 for r in rows], np.uint8),
                    lambda_end=np.array([r["lambda_end"] for r in rows]))
    return leg


def disk_distance(x, disk=DISK):
    rc = np.hypot(x[:, 1], x[:, 2])
    return np.maximum(np.maximum(np.abs(x[:, 3]) - disk[0], disk[1] - rc), rc - disk[2])


@functools.lru_cache(maxsize=None)
def oracle_kerr_chain():
    metric, objs = kerr_scene()
    s0 = cpu_states(metric, observer(), *SIZES[0])
    return s0, chain(oracle_leg(metric, solver()), s0, objs, 3)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_exported():
    assert set(ORD_EXPORTS) <= set(abi.EXPORTS)
    lib = abi.load()
    hdr = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    for s in ORD_EXPORTS:
        assert hasattr(lib, s), s
        assert s + "(" in hdr, s
    assert "#define RTGR_ABI_VERSION 4" in hdr and lib.rtgr_abi_version() == 4     # additive: no existing layout moved
    assert {"DiskOrders", "trace_orders"} <= set(rt.api.__all__)
    jl = open(os.path.join(ROOT, "julia", "RayTraceGRHIP.jl")).read()
    for s in ORD_EXPORTS:   # the Julia module binds the host-pointer entries only, as for every feature
        assert ("_device_" in s) != (f"ccall((:{s}, librtgr)" in jl), s
    for word in ("struct RtgrDiskOrders", "struct RtgrOrderPlanes", "function DiskOrders(", "function trace_rays_orders(",
                 "#   RtgrDiskOrders 32   max_order 0, flags 4, margin 8, transmission 16, pad 24"):
        assert word in jl, word


def test_struct_layout_ctypes_and_c(tmp_path):
    s = abi.rtgr_disk_orders
    assert C.sizeof(s) == 32 and [getattr(s, f).offset for f in ("max_order", "flags", "margin", "transmission", "pad")] == [0, 4, 8, 16, 24]
    p = abi.rtgr_order_planes
    assert C.sizeof(p) == 48 and [getattr(p, f).offset for f in ("count", "hit32", "state_end", "g", "rgb_order", "state0")] == [0, 8, 16, 24, 32, 40]
    exe = str(tmp_path / "orders_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "orders_layout.c"), "-o", exe])
    assert subprocess.check_output([exe]).split() == [b"32", b"0", b"4", b"8", b"16", b"24", b"48", b"0", b"8", b"16", b"24", b"32", b"40"]
    o = rt.DiskOrders(3, 0.5)
    assert (o.max_order, o.flags, o.margin, o.transmission, o.pad) == (3, 0, 0.0, 0.5, 0)


def test_oracle_chain_crossing_legs_end_on_the_inflated_disk():
    """The construction itself, on the CPU oracle, for the observer's own states at 64 x 48 (N = 3): every crossing leg ends as an event on
    D+ — object 1 of S+ — at distance eta = 0.025 from D to 1e-12, in at most 40 accepted steps.  And the numbers test_enough_to_see
    relies on, confirmed here for the observer's states: the frame holds the whole disk (no disk pixel on its border rows and columns)
    and has 105 order-1 and 4 order-2 pixels, none of order 3 (the issue's plane camera: 234, 9, 0)."""
    s0, (leg0, orders) = oracle_kerr_chain()
    n0 = int((leg0["hit"] == DISK_OBJECT).sum())
    reach = [int((o["cont"]["hit"] == DISK_OBJECT).sum()) if o["cont"] is not None else 0 for o in orders]
    h = (leg0["hit"] == DISK_OBJECT).reshape(SIZES[0][1], SIZES[0][0])
    print("order 0:", n0, "orders 1..:", reach, "disk pixels on the border:", int(h[0].sum() + h[-1].sum() + h[:, 0].sum() + h[:, -1].sum()))
    assert not (h[0].any() or h[-1].any() or h[:, 0].any() or h[:, -1].any()), "the frame does not hold the whole disk"
    assert n0 >= 1000 and reach[0] >= 100 and reach[1] >= 4
    for o in orders:
        cr = o["cross"]
        assert cr["go"].all(), "a crossing leg did not end as an event on D+"
        d = disk_distance(cr["state_end"])
        print("crossing legs:", len(d), "max |d - eta|", np.abs(d - ETA).max(), "max steps", cr["n_accept"].max())
        assert np.abs(d - ETA).max() <= 1e-12
        assert cr["n_accept"].max() <= 40


def test_the_stored_truth_chains_are_true():
    """tests/golden/truth_orders.npz holds, for the pixels of test_true_geodesics, the observer's state and the end state of each order by
    DOP853 chained through S and S+ (max_step 0.05), and the oracle's chain beside it.  One order-1 pixel is integrated again here: the
    file is what its recipe gives."""
    G = np.load(GOLDEN)
    metric, objs = kerr_scene()
    s0 = cpu_states(metric, observer(), *SIZES[0])
    assert np.abs(s0[G["pixel"]] - G["s0"]).max() <= 1e-14
    q = int(np.flatnonzero(G["order"] == 1)[0])
    _, orders = chain(truth_leg(metric, solver()), G["s0"][q:q + 1], objs, 1)
    assert orders[0]["cont"]["hit"][0] == DISK_OBJECT
    assert np.abs(orders[0]["cont"]["state_end"][0] - G["truth_end"][q]).max() <= 1e-12


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


def api_leg(lib, metric, opt, dtype, counters):
    """rtgr_trace_f64 / _f32 fed caller-supplied states (host pointers); the counters of every leg are appended to `counters`"""
    def leg(objs, states):
        sc, m = rt.make_scene(metric, objs), len(states)
        st = np.ascontiguousarray(states, dtype)
        out = dict(rgb=np.zeros((3, m), dtype), state_end=np.zeros((m, 8), dtype), hit=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
        o = abi.rtgr_ray_outputs(state_end=out["state_end"].ctypes.data, hit32=out["hit"].ctypes.data, status=out["status"].ctypes.data)
        ctr = abi.rtgr_counters()
        fn = lib.rtgr_trace_f64 if dtype == np.float64 else lib.rtgr_trace_f32
        abi.check(lib, fn(None, C.byref(sc), C.byref(opt), st.ctypes.data, None, m, 1, 0, 1, out["rgb"].ctypes.data, C.byref(o), C.byref(ctr)))
        counters.append(ctr.as_dict())
        return out
    return leg


def api_chain(lib, metric, objs, ob, s0, N, T, dtype, opt, em):
    """What rtgr_trace_orders_* must give, spelled out through the public API: rtgr_trace_* with state0 through S, S+, S, ...,
    rt.eval_disk_emission under the observer, the accumulation in numpy in the entry's scalar type"""
    n, counters = len(s0), []
    leg0, orders = chain(api_leg(lib, metric, opt, dtype, counters), s0, objs, N)
    nan = dtype(np.nan)
    P = dict(hit32=np.zeros((N + 1, n), np.uint32), state_end=np.full((N + 1, n, 8), nan, dtype), g=np.full((N + 1, n), nan, dtype),
             rgb_order=np.full((N + 1, 3, n), nan, dtype), count=np.zeros(n, np.uint8), state0=np.ascontiguousarray(s0, dtype))
    emit = lambda idx, se: rt.eval_disk_emission(metric, objs, em, P["state0"][idx], se, dtype=dtype, observer=ob)
    on0 = np.flatnonzero(leg0["hit"] == DISK_OBJECT)
    rgb = leg0["rgb"].copy()
    E = emit(on0, leg0["state_end"][on0])
    rgb[:, on0] = E["rgb"].T
    P["hit32"][0], P["state_end"][0], P["g"][0, on0], P["rgb_order"][0], P["count"][on0] = leg0["hit"], leg0["state_end"], E["g"], rgb, 1
    t = dtype(T)
    for k, o in enumerate(orders, start=1):
        if o["cont"] is None:
            break
        idx, cont = o["idx"], o["cont"]
        on = cont["hit"] == DISK_OBJECT
        col = cont["rgb"].copy()
        if on.any():
            E = emit(idx[on], cont["state_end"][on])
            col[:, on] = E["rgb"].T
            P["g"][k, idx[on]] = E["g"]
        prod = (t * col).astype(dtype)
        rgb[:, idx] = (rgb[:, idx] + prod).astype(dtype)
        P["hit32"][k, idx[on]] = DISK_OBJECT
        P["state_end"][k, idx[on]] = cont["state_end"][on]
        P["rgb_order"][k][:, idx[on]] = col[:, on]
        P["count"][idx[on]] += 1
        t = dtype(t * dtype(T))
    P["rgb"] = rgb
    P["counters"] = {f: sum(c[f] for c in counters) for f in counters[0]}
    P["per_leg_rays"] = [c["rays"] for c in counters]
    return P


PLANES = ("rgb", "count", "hit32", "state_end", "g", "rgb_order", "state0")


def same(a, b):
    """equal to the bit; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and a[~na].tobytes() == b[~nb].tobytes()


def assert_same_planes(got, want, what):
    for k in PLANES:
        assert same(got[k], want[k]), f"{what}: plane {k} differs"


def device_call(lib, dtype, metric, objs, ob, ni, nj, em, orders, opt, stream=None, s0=None):
    """rtgr_trace_orders_device_*: every plane on the device (torch), read back -> the dict of the host entry"""
    import torch
    tt = torch.float64 if dtype == np.float64 else torch.float32
    n, nb = ni * nj, orders.max_order + 1
    sc = rt.make_scene(metric, objs)
    T = dict(rgb=torch.full((3, n), 7.0, dtype=tt, device="cuda"), count=torch.full((n,), 7, dtype=torch.uint8, device="cuda"),
             hit32=torch.full((nb, n), 7, dtype=torch.int32, device="cuda"), state_end=torch.full((nb, n, 8), 7.0, dtype=tt, device="cuda"),
             g=torch.full((nb, n), 7.0, dtype=tt, device="cuda"), rgb_order=torch.full((nb, 3, n), 7.0, dtype=tt, device="cuda"),
             state0=torch.full((n, 8), 7.0, dtype=tt, device="cuda"))
    d_s0 = None if s0 is None else torch.from_numpy(np.ascontiguousarray(s0, dtype)).cuda()
    torch.cuda.synchronize()
    planes = abi.rtgr_order_planes(**{k: T[k].data_ptr() for k in T if k != "rgb"})
    ctr = abi.rtgr_counters()
    fn = getattr(lib, "rtgr_trace_orders_device_" + ("f64" if dtype == np.float64 else "f32"))
    abi.check(lib, fn(None, C.byref(sc), C.byref(opt), None if ob is None else C.byref(ob), None if d_s0 is None else d_s0.data_ptr(), ni, nj, None,
                      C.byref(em), C.byref(orders), T["rgb"].data_ptr(), C.byref(planes), C.byref(ctr), stream))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in T.items()}
    res["hit32"] = res["hit32"].view(np.uint32)
    res["counters"] = ctr.as_dict()
    return res


_FRAMES = {}


def host_frame(dtype, size, N=2, T=0.5, batch=0, textures=None):
    key = (np.dtype(dtype).name, size, N, T, batch, textures is not None)
    if key not in _FRAMES:
        metric, objs = kerr_scene()
        _FRAMES[key] = rt.trace_orders(metric, objs, observer(batch), size[0], size[1], emission(), rt.DiskOrders(N, T), opt=solver(dtype), dtype=dtype,
                                       textures=textures)
    return _FRAMES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("size", SIZES)
def test_bit_for_bit_against_the_chain_through_the_public_api(lib, dtype, size):
    """N = 2, T = 0.5, eta default: every plane, count, rgb and the sum of the legs' counters equal the chain rt.make_observer_canvas ->
    rtgr_trace_* with state0 through S, S+, S, ... -> rt.eval_disk_emission with the observer -> the numpy accumulation, to the bit; at
    37 x 19 in chunks of five rows.  The same on a side stream, after rtgr_trim, and for the device entry against the host entry."""
    import torch
    ni, nj = size
    batch = 5 * ni if size == SIZES[1] else 0
    metric, objs = kerr_scene()
    ob, em, orders, opt = observer(batch), emission(), rt.DiskOrders(2, 0.5), solver(dtype)
    s0 = rt.make_observer_canvas(metric, objs, ob, ni, nj, dtype=dtype)
    want = api_chain(lib, metric, objs, ob, s0, 2, 0.5, dtype, opt, em)
    print("rays per leg:", want["per_leg_rays"], "crossings:", np.bincount(want["count"]))
    host = host_frame(dtype, size, batch=batch)
    assert_same_planes(host, want, "host entry")
    assert host["counters"] == want["counters"]
    dev = device_call(lib, dtype, metric, objs, ob, ni, nj, em, orders, opt)
    assert_same_planes(dev, host, "device entry, default stream")
    assert dev["counters"] == want["counters"]
    side = torch.cuda.Stream()
    dev = device_call(lib, dtype, metric, objs, ob, ni, nj, em, orders, opt, stream=side.cuda_stream)
    assert_same_planes(dev, host, "device entry, side stream")
    abi.check(lib, lib.rtgr_trim(None))
    dev = device_call(lib, dtype, metric, objs, ob, ni, nj, em, orders, opt, stream=side.cuda_stream)
    assert_same_planes(dev, host, "device entry after rtgr_trim")
    again = rt.trace_orders(metric, objs, ob, ni, nj, em, orders, opt=opt, dtype=dtype)
    assert_same_planes(again, host, "host entry after rtgr_trim")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("sky", [False, True], ids=["plain", "sky-texture"])
def test_order_zero_and_opaque_disk_equal_the_emitted_observer_frame(lib, dtype, sky):
    """Block 0 of every plane and the T = 0 picture equal rtgr_trace_observer_* with emit, with and without a texture bound to the sky.
    (The picture numerically: a -0 channel of a continuing pixel becomes +0, the one exception the header states.)"""
    ni, nj = SIZES[1]
    metric, objs = kerr_scene()
    ob, em, opt = observer(), emission(), solver(dtype)
    tex = None
    if sky:
        yy, xx = np.mgrid[0:16, 0:32]
        tex = {1: rt.texture_load(np.stack([xx / 31.0, yy / 15.0, 0.25 + 0 * xx]))}
    try:
        ref = rt.trace_observer(metric, objs, ob, ni, nj, emission=em, textures=tex, opt=opt, dtype=dtype, details=True)
        for T in (0.0, 0.5):
            got = rt.trace_orders(metric, objs, ob, ni, nj, em, rt.DiskOrders(2, T), textures=tex, opt=opt, dtype=dtype)
            assert same(got["rgb_order"][0], ref["rgb"]) and same(got["g"][0], ref["g"]) and same(got["state_end"][0], ref["state_end"])
            assert same(got["hit32"][0], ref["hit"].astype(np.uint32))
            assert same(got["state0"], rt.make_observer_canvas(metric, objs, ob, ni, nj, dtype=dtype))
            assert got["counters"]["rays"] >= ref["counters"]["rays"]
            if T == 0.0:
                assert np.array_equal(got["rgb"], ref["rgb"])
                off = got["count"] == 0
                assert same(got["rgb"][:, off], ref["rgb"][:, off])
            else:
                assert not np.array_equal(got["rgb"], ref["rgb"])
    finally:
        if tex:
            rt.texture_unload(tex[1])


@pytest.mark.gpu
def test_enough_to_see(lib):
    """At 64 x 48 the frame has at least 100 order-1 and at least 4 order-2 pixels.  The CPU oracle's chain over the observer's own
    states gives 105 and 4 (test_oracle_chain_crossing_legs_end_on_the_inflated_disk); the issue's plane camera gave 234 and 9.  (A
    perspective frame wide enough for the disk, 1.4 x 1.05 rad, has 70 and 5: hence the equirectangular frame of observer().)"""
    f = host_frame(np.float64, SIZES[0])
    n1, n2 = int((f["hit32"][1] == DISK_OBJECT).sum()), int((f["hit32"][2] == DISK_OBJECT).sum())
    print("order 1:", n1, "order 2:", n2, "crossings:", np.bincount(f["count"]))
    assert ((f["count"] >= 2) == (f["hit32"][1] == DISK_OBJECT)).all() and ((f["count"] >= 3) == (f["hit32"][2] == DISK_OBJECT)).all()
    assert np.isnan(f["state_end"][1][f["hit32"][1] == 0]).all() and np.isfinite(f["state_end"][1][f["hit32"][1] == DISK_OBJECT]).all()
    assert n1 >= 100 and n2 >= 4


@pytest.mark.gpu
def test_true_geodesics(lib):
    """For 4 order-1 and 2 order-2 pixels spread in rho (evenly spaced in the order of rho among the pixels of each order), the device's
    end state of that order must lie within max(3e-11, 4 x the CPU oracle's own error on that pixel) of DOP853 chained through S and S+
    with max_step 0.05 (stored: tests/golden/truth_orders.npz, made by tests/golden/make_orders_truth.py and spot-checked by
    test_the_stored_truth_chains_are_true; the device's start states equal the stored ones to 1e-14).
    Measured on an MI355X, max |end - truth| over the 8 components, oracle / device / bound:
        order 1  pixel 1368 rho  3.00   2.20e-11 / 7.33e-12 / 8.8e-11
                 pixel 2090 rho  4.52   4.57e-11 / 4.38e-11 / 1.8e-10
                 pixel  740 rho  6.77   2.31e-11 / 1.52e-11 / 9.3e-11
                 pixel  677 rho 11.96   8.65e-11 / 4.98e-11 / 3.5e-10
        order 2  pixel 2027 rho  4.11   1.27e-09 / 1.32e-09 / 5.1e-09
                 pixel 1132 rho 10.44   1.68e-09 / 1.01e-09 / 6.7e-09
    The oracle's error carries the ring's amplification, the factor 4 the contraction differences between oracle and device."""
    G = np.load(GOLDEN)
    f = host_frame(np.float64, SIZES[0])
    assert np.abs(f["state0"][G["pixel"]] - G["s0"]).max() <= 1e-14
    assert (G["order"] == 1).sum() >= 4 and (G["order"] == 2).sum() >= 2
    rho = np.hypot(G["truth_end"][:, 1], G["truth_end"][:, 2])
    for k in (1, 2):
        assert np.ptp(rho[G["order"] == k]) >= 1.0, "the pixels are not spread in rho"
    missed = []
    for q, (p, k) in enumerate(zip(G["pixel"], G["order"])):
        assert f["hit32"][k, p] == DISK_OBJECT
        e_dev = np.abs(f["state_end"][k, p] - G["truth_end"][q]).max()
        e_orc = np.abs(G["oracle_end"][q] - G["truth_end"][q]).max()
        bound = max(TRUTH_BOUND, 4 * e_orc)
        print(f"pixel {p} order {k} rho {rho[q]:.3f}: oracle {e_orc:.2e} device {e_dev:.2e} bound {bound:.2e}")
        if not e_dev <= bound:
            missed.append((int(p), int(k), float(e_dev), float(bound)))
    assert not missed, missed


@pytest.mark.gpu
def test_the_rings_are_where_they_must_be(lib):
    """The Schwarzschild strip through state0 with obs = NULL, N = 3: every ray that crosses the disk at least twice has 5.02 < b < 6.17
    (the lensing ring, Gralla, Holz & Wald 2019), every ray that crosses it at least three times 5.19 < b < 5.23 (the photon ring); at
    least 50 of the first and 3 of the second (the oracle chain: 101 and 4)."""
    metric = rt.KerrSchild(1.0, 0.0)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -80.0), rt.Disk(*DISK)]
    s0, b = strip_states(metric)
    f = rt.trace_orders(metric, objs, None, len(s0), 1, emission(), rt.DiskOrders(3, 1.0), state0=s0, opt=solver(lambda1=400.0))
    two, three = f["count"] >= 2, f["count"] >= 3
    print("count >= 2:", two.sum(), b[two].min(), b[two].max(), "count >= 3:", three.sum(), b[three].min(), b[three].max())
    assert two.sum() >= 50 and three.sum() >= 3
    assert (b[two] > 5.02).all() and (b[two] < 6.17).all()
    assert (b[three] > 5.19).all() and (b[three] < 5.23).all()
    assert same(f["state0"], s0)


@pytest.mark.gpu
def test_composition_with_the_stages(lib):
    """Block k of the planes fed to rtgr_spectrum_device_* and rtgr_polarization_device_* gives what the same stage gives on planes built
    by hand from the chain, to the bit; and along the truth chain of one order-1 pixel rt.eval_walker_penrose at the observer and at the
    order-1 end agree to the conservation bound of tests/test_polarization.py (1e-9)."""
    import torch
    dtype, (ni, nj) = np.float64, SIZES[0]
    n = ni * nj
    metric, objs = kerr_scene()
    ob, em, opt = observer(), emission(), solver(dtype)
    sc = rt.make_scene(metric, objs)
    f = host_frame(dtype, SIZES[0])
    s0 = rt.make_observer_canvas(metric, objs, ob, ni, nj, dtype=dtype)
    hand = api_chain(lib, metric, objs, ob, s0, 2, 0.5, dtype, opt, em)
    spec = rt.Spectrum("line", 0.3, 1.5, 24, rho_min=DISK[1], rho_max=DISK[2])
    pol = rt.Polarization("scatter", 0.12, 0.4)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for k in (1, 2):
        outs = []
        for src in (f, hand):
            hit, se, g, st0 = dev(src["hit32"][k].view(np.int32)), dev(src["state_end"][k]), dev(src["g"][k]), dev(src["state0"])
            table = torch.zeros((24, 3), dtype=torch.float64, device="cuda")
            q, u = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
            abi.check(lib, lib.rtgr_spectrum_device_f64(None, C.byref(sc), C.byref(em), C.byref(spec), C.byref(ob), ni, nj, hit.data_ptr(), se.data_ptr(),
                                                        g.data_ptr(), table.data_ptr(), None))
            abi.check(lib, lib.rtgr_polarization_device_f64(None, C.byref(sc), C.byref(em), C.byref(pol), C.byref(ob), ni, nj, hit.data_ptr(), st0.data_ptr(),
                                                            se.data_ptr(), q.data_ptr(), u.data_ptr(), None, None))
            torch.cuda.synchronize()
            outs.append((table.cpu().numpy(), q.cpu().numpy(), u.cpu().numpy()))
        assert outs[0][0].sum() > 0 and np.isfinite(outs[0][1]).sum() == (f["hit32"][k] == DISK_OBJECT).sum()
        for a, b in zip(*outs):
            assert same(a, b), k
    # the constants are conserved across the crossings: the two ends of one order-1 pixel's truth chain, with a vector f carried along the
    # same geodesic by the truth side's parallel transporter (stored with the chain)
    G = np.load(GOLDEN)
    ends = np.stack([G["s0"][int(G["wp_row"])], G["truth_end"][int(G["wp_row"])]])
    kap = rt.eval_walker_penrose(metric, objs, ends, np.stack([G["wp_f0"], G["wp_f1"]]))
    print("kappa at the observer", kap[0], "at the order-1 end", kap[1])
    assert np.isfinite(kap).all() and np.abs(kap[0]).max() > 1e-3
    assert np.abs(kap[1] - kap[0]).max() <= 1e-9


def _refusals():
    """(what it is, keyword overrides of the call, words of the message)"""
    nan, inf = float("nan"), float("inf")
    O = lambda **kw: abi.rtgr_disk_orders(**dict(dict(max_order=2, flags=0, margin=0.0, transmission=0.5, pad=0), **kw))
    return [("N = 0", dict(orders=O(max_order=0)), b"max_order"), ("N = 9", dict(orders=O(max_order=9)), b"max_order"),
            ("eta NaN", dict(orders=O(margin=nan)), b"margin"), ("eta inf", dict(orders=O(margin=inf)), b"margin"),
            ("eta < 0", dict(orders=O(margin=-0.01)), b"margin"), ("eta >= r_in", dict(orders=O(margin=3.0)), b"r_in"),
            ("T < 0", dict(orders=O(transmission=-0.1)), b"transmission"), ("T > 1", dict(orders=O(transmission=1.5)), b"transmission"),
            ("T NaN", dict(orders=O(transmission=nan)), b"transmission"), ("flags", dict(orders=O(flags=1)), b"flags"),
            ("pad", dict(orders=O(pad=1)), b"pad"), ("no orders", dict(orders=None), b"rtgr_disk_orders is NULL"),
            ("no emit", dict(em=None), b"rtgr_disk_emission is NULL"), ("no observer, no states", dict(ob=None), b"rtgr_observer is NULL"),
            ("emit names the sky", dict(em=rt.DiskEmission(1, T_FRAME)), b"only a Disk emits"),
            ("emitter's T_in", dict(em=rt.DiskEmission(DISK_OBJECT, -1.0)), b"T_in"),
            ("observer's fov", dict(ob=rt.Observer((0, 0, -18, 9), (0, 0, 18, -9), (0, 0, 0, 1), 4.0, 1.0)), b"fov"),
            ("empty canvas", dict(ni=0), b"bad canvas"), ("no rgb", dict(rgb=None), b"rgb is NULL")]


@pytest.mark.gpu
def test_refusals(lib):
    """Each item of the refused list, by its message, through the host and the device entry; the outputs are not written; a stream under
    capture is refused and the capture survives."""
    import torch
    from test_polarization import _hip_runtime
    ni, nj = 8, 6
    n = ni * nj
    metric, objs = kerr_scene()
    sc, opt = rt.make_scene(metric, objs), solver()
    ref = lambda x: None if x is None else C.byref(x)
    rgb_h, rgb_d = np.full((3, n), 7.0), torch.full((3, n), 7.0, dtype=torch.float64, device="cuda")
    base = dict(ob=observer(), em=emission(), orders=rt.DiskOrders(2, 0.5), ni=ni, rgb=True)

    def call(device, stream=None, **kw):
        a = dict(base, **kw)
        rgb = None if a["rgb"] is None else (rgb_d.data_ptr() if device else rgb_h.ctypes.data)
        fn = lib.rtgr_trace_orders_device_f64 if device else lib.rtgr_trace_orders_f64
        args = [None, C.byref(sc), C.byref(opt), ref(a["ob"]), None, a["ni"], nj, None, ref(a["em"]), ref(a["orders"]), rgb, None, None]
        return fn(*(args + [stream] if device else args)), lib.rtgr_last_error()

    for what, kw, words in _refusals():
        for device in (False, True):
            rc, msg = call(device, **kw)
            assert rc == abi.ERR_BAD_ARG and words in msg, (what, device, rc, msg)
    # a 4-D grid and a user metric are the emitted observer trace's refusals (tests/test_emission.py, tests/test_observer.py hold them)
    side = torch.cuda.Stream()
    assert call(True, side.cuda_stream)[0] == 0          # (workspace and scratch exist before the capture)
    torch.cuda.synchronize()
    rgb_d.fill_(7.0)
    torch.cuda.synchronize()
    hip, graph = _hip_runtime(), C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 2) == 0
    rc, msg = call(True, side.cuda_stream)
    assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
    assert rc == abi.ERR_BAD_ARG and b"captured" in msg and b"rtgr_trace_orders" in msg, msg
    if graph.value:
        hip.hipGraphDestroy(graph)
    torch.cuda.synchronize()
    assert bool((rgb_d == 7.0).all()) and (rgb_h == 7.0).all()
