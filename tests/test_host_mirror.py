"""The blocking host-pointer calls (make_canvas, the rtgr_eval_* hooks, the planes of rtgr_trace_polarized_* and rtgr_trace_orders_*) against
the contract of their arrays, which the other tests only exercise by accident because rt.api always hands over exact-size arrays: an output
of `count` elements gets exactly `count` elements written — no byte behind them, none of them left out —, an omitted optional output changes
no other, n = 0 touches nothing, and rtgr_eval_texture_*'s rgb goes up as well as down.  The library is called through ctypes directly.

Every hook runs at n = 257 points (one full block of 256 threads plus one) of a valid scene: Kerr (RTGR_KS_TRUE, a = 0.5) with one Disk, the
points taken from the start and end states of a 17 x 17 frame of it.  Conditions on bits: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from scenes import rt

abi = rt._abi
N = 257
GUARD = 64          # bytes behind every output array
PAT = 0xA5          # … and what they, and the array, hold before the call (as a double: -8.7e-129, as a float: -2.9e-16, no NaN)
DTYPES = (np.float64, np.float32)
T_IN = 30000.0


class Out:
    """an output array of `count` elements handed over GUARD bytes longer than that, every byte PAT"""

    def __init__(self, dtype, count):
        self.dtype, self.count = np.dtype(dtype), int(count)
        self.nbytes = self.count * self.dtype.itemsize
        self.raw = np.full(self.nbytes + GUARD, PAT, np.uint8)

    @property
    def ptr(self):
        return self.raw.ctypes.data

    def bits(self):
        return self.raw[:self.nbytes].tobytes()

    def guard_intact(self):
        return bool((self.raw[self.nbytes:] == PAT).all())

    def elements_left(self):
        """how many whole elements still hold the pattern"""
        return int((self.raw[:self.nbytes].reshape(self.count, self.dtype.itemsize) == PAT).all(axis=1).sum())

    def untouched(self):
        return bool((self.raw == PAT).all())


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


def scene():
    return rt.make_scene(rt.KerrSchild(1, 0.5), [rt.Disk(0.05, 4.5, 8.0)])


def observer():
    pos = (0, 0, -12, 8)
    return rt.Observer(pos, (0, -pos[1], -pos[2], -pos[3]), (0, 0, 0, 1), 1.3, 0.9)


def emission():
    return rt.DiskEmission(1, T_IN)


_POINTS = {}


def points(lib, dtype):
    """the first N start and end states of the 17 x 17 frame (computed once per scalar type, read only), and what the hooks take of them: an
    end state that is not finite (a ray lost in the hole) gives way to its start state, so that every input is a number"""
    key = np.dtype(dtype).name
    if key not in _POINTS:
        suf = "f64" if dtype == np.float64 else "f32"
        sc, ob, em, opt = scene(), observer(), emission(), rt.solver_defaults(dtype)
        ni = nj = 17
        s0 = np.zeros((ni * nj, 8), dtype)
        abi.check(lib, getattr(lib, "rtgr_make_observer_canvas_" + suf)(None, C.byref(sc), C.byref(ob), ni, nj, 0, nj, s0.ctypes.data))
        rgb, g, se = np.zeros((3, ni * nj), dtype), np.zeros(ni * nj, dtype), np.zeros((ni * nj, 8), dtype)
        outs = abi.rtgr_ray_outputs(state_end=se.ctypes.data)
        abi.check(lib, getattr(lib, "rtgr_trace_observer_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, None, C.byref(em), rgb.ctypes.data,
                                                                  C.byref(outs), g.ctypes.data, None))
        s0, se = s0[:N].copy(), se[:N].copy()
        bad = ~np.isfinite(se).all(axis=1)
        se[bad] = s0[bad]
        d = se[:, 1:4].copy()
        d[np.linalg.norm(d, axis=1) == 0] = (1, 0, 0)
        P = dict(s0=s0, se=se, x=se[:, :4].copy(), dir=d, f=np.roll(se[:, 4:8], 1, axis=1).copy(),
                 xyt=np.stack([se[:, 1], se[:, 2], se[:, 0]], axis=1).copy(),
                 xyg=np.stack([se[:, 1], se[:, 2], np.linspace(0.5, 1.2, N).astype(dtype)], axis=1).copy(),
                 pos=np.linspace(0.5, 50.0, N))
        for v in P.values():
            v.setflags(write=False)
        _POINTS[key] = P
    return _POINTS[key]


_TEXTURE = []


def texture(lib):
    if not _TEXTURE:
        texels = np.linspace(0.1, 0.9, 3 * 2 * 4).reshape(3, 2, 4)
        desc, tid = abi.rtgr_texture_desc(width=4, height=2, flags=0, pad=0), C.c_uint64(0)
        abi.check(lib, lib.rtgr_texture_load(None, C.byref(desc), texels.ctypes.data, C.byref(tid)))
        _TEXTURE.append(tid.value)
    return _TEXTURE[0]


# ---- the calls: name -> (outputs, call).  outputs: {name: (dtype or "R" for the call's scalar type, elements as a function of n, optional)};
# call(lib, suf, P, n, p) with p[name] the pointer of each output (None: omitted) -> the status.  `frame`: the call has no n of its own (a
# canvas of N x 1 pixels, or one record): left out of the n = 0 test
class Hook:
    def __init__(self, outputs, call, frame=False, f64_only=False):
        self.outputs, self.call, self.frame, self.f64_only = outputs, call, frame, f64_only


def _camera():
    return rt.make_camera((0, 4, -2, 0), (0, 1, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0))


def _sc(x):
    return C.byref(x)


def _make_canvas(lib, suf, P, n, p):
    sc, cam = scene(), _camera()
    return getattr(lib, "rtgr_make_canvas_" + suf)(None, _sc(sc), _sc(cam), N, 1, 0, 1, p["state0"])


def _eval_metric(lib, suf, P, n, p):
    sc = scene()
    return getattr(lib, "rtgr_eval_metric_" + suf)(None, _sc(sc), P["x"].ctypes.data, n, p["g"], p["dg"], p["Gam"])


def _eval_geodesic(path):
    def call(lib, suf, P, n, p):
        sc = scene()
        return getattr(lib, "rtgr_eval_geodesic_" + suf)(None, _sc(sc), P["se"].ctypes.data, n, path, p["ds"])
    return call


def _eval_objects(lib, suf, P, n, p):
    sc, opt = scene(), rt.solver_defaults(np.float64 if suf == "f64" else np.float32)
    return getattr(lib, "rtgr_eval_objects_" + suf)(None, _sc(sc), _sc(opt), P["x"].ctypes.data, n, p["d"], p["dmin"], p["hit"], p["rgb"])


def _eval_fastmath(lib, suf, P, n, p):
    return lib.rtgr_eval_fastmath_f64(None, P["pos"].ctypes.data, n, p["rcp"], p["rsq"])


def _eval_texture(lib, suf, P, n, p):
    return getattr(lib, "rtgr_eval_texture_" + suf)(None, texture(lib), abi.TEX_BILINEAR, P["dir"].ctypes.data, n, None, p["rgb"])


def _eval_emission(lib, suf, P, n, p):
    sc, em, ob = scene(), emission(), observer()
    return getattr(lib, "rtgr_eval_disk_emission_observer_" + suf)(None, _sc(sc), _sc(em), _sc(ob), P["s0"].ctypes.data, P["se"].ctypes.data, n, p["omega"],
                                                                  p["u_emit"], p["g"], p["rgb"])


def _make_observer_canvas(lib, suf, P, n, p):
    sc, ob = scene(), observer()
    return getattr(lib, "rtgr_make_observer_canvas_" + suf)(None, _sc(sc), _sc(ob), N, 1, 0, 1, p["state0"])


def _eval_observer(lib, suf, P, n, p):
    sc, ob = scene(), observer()
    return getattr(lib, "rtgr_eval_observer_" + suf)(None, _sc(sc), _sc(ob), p["frame"], p["omega"], C.cast(p["valid"], C.POINTER(C.c_int)))


def _eval_hot_spot(lib, suf, P, n, p):
    sc, em, spot = scene(), emission(), rt.HotSpot(6.0, 0.5)
    return getattr(lib, "rtgr_eval_hot_spot_" + suf)(None, _sc(sc), _sc(em), _sc(spot), P["xyt"].ctypes.data, n, p["omega_s"],
                                                    C.cast(p["valid"], C.POINTER(C.c_int)), p["j"])


LINE = dict(kind="line", lo=0.3, hi=1.5, nb=16, rho_min=4.5, rho_max=8.0)
THERMAL = dict(kind="thermal", lo=1e3, hi=1e5, nb=5, log=True)


def _eval_spectrum(spec):
    def call(lib, suf, P, n, p):
        sc, em, sp = scene(), emission(), rt.Spectrum(**spec)
        return getattr(lib, "rtgr_eval_spectrum_" + suf)(None, _sc(sc), _sc(em), _sc(sp), P["xyg"].ctypes.data, n, p["axis"], p["bin"], p["val"])
    return call


def _eval_polarization(lib, suf, P, n, p):
    sc, em, ob, pol = scene(), emission(), observer(), rt.Polarization("scatter", 0.12, 0.4)
    return getattr(lib, "rtgr_eval_polarization_" + suf)(None, _sc(sc), _sc(em), _sc(pol), _sc(ob), P["s0"].ctypes.data, P["se"].ctypes.data, n, p["kappa"],
                                                        p["f_em"], p["aux"], p["delta"], p["q"], p["u"], p["valid"])


def _eval_walker_penrose(lib, suf, P, n, p):
    sc = scene()
    return getattr(lib, "rtgr_eval_walker_penrose_" + suf)(None, _sc(sc), P["se"].ctypes.data, P["f"].ctypes.data, n, p["kappa"])


def _trace_polarized(lib, suf, P, n, p):
    sc, em, ob, pol = scene(), emission(), observer(), rt.Polarization("scatter", 0.12, 0.4)
    opt = rt.solver_defaults(np.float64 if suf == "f64" else np.float32)
    return getattr(lib, "rtgr_trace_polarized_" + suf)(None, _sc(sc), _sc(opt), _sc(ob), N, 1, None, _sc(em), _sc(pol), p["rgb"], None, p["g"], p["q"], p["u"],
                                                      p["aux"], None)


ORDERS = 2   # N of rtgr_disk_orders: N + 1 blocks in the per-order planes


def _trace_orders(given_state0):
    def call(lib, suf, P, n, p):
        sc, em, ob, orders = scene(), emission(), observer(), rt.DiskOrders(ORDERS)
        opt = rt.solver_defaults(np.float64 if suf == "f64" else np.float32)
        planes = abi.rtgr_order_planes(count=p["count"], hit32=p["hit32"], state_end=p["state_end"], g=p["g"], rgb_order=p["rgb_order"], state0=p["state0"])
        s0 = None
        if given_state0:   # the N x 1 canvas' own states, from the hook
            s0 = np.zeros((N, 8), np.float64 if suf == "f64" else np.float32)
            abi.check(lib, getattr(lib, "rtgr_make_observer_canvas_" + suf)(None, _sc(sc), _sc(ob), N, 1, 0, 1, s0.ctypes.data))
        return getattr(lib, "rtgr_trace_orders_" + suf)(None, _sc(sc), _sc(opt), _sc(ob), None if s0 is None else s0.ctypes.data, N, 1, None, _sc(em),
                                                       _sc(orders), p["rgb"], _sc(planes), None)
    return call


ORDER_PLANES = dict(rgb=("R", lambda n: 3 * n, False), count=(np.uint8, lambda n: n, True), hit32=(np.uint32, lambda n: (ORDERS + 1) * n, True),
                    state_end=("R", lambda n: (ORDERS + 1) * n * 8, True), g=("R", lambda n: (ORDERS + 1) * n, True),
                    rgb_order=("R", lambda n: (ORDERS + 1) * 3 * n, True), state0=("R", lambda n: n * 8, True))
HOOKS = {
    "make_canvas": Hook(dict(state0=("R", lambda n: N * 8, False)), _make_canvas, frame=True),
    "eval_metric": Hook(dict(g=("R", lambda n: 16 * n, True), dg=("R", lambda n: 64 * n, True), Gam=("R", lambda n: 64 * n, True)), _eval_metric),
    "eval_geodesic_path0": Hook(dict(ds=("R", lambda n: 8 * n, False)), _eval_geodesic(0)),
    "eval_geodesic_path2": Hook(dict(ds=("R", lambda n: 8 * n, False)), _eval_geodesic(2)),
    "eval_objects": Hook(dict(d=("R", lambda n: n, True), dmin=("R", lambda n: n, True), hit=(np.uint8, lambda n: n, True), rgb=("R", lambda n: 3 * n, True)),
                         _eval_objects),
    "eval_fastmath": Hook(dict(rcp=(np.float64, lambda n: n, True), rsq=(np.float64, lambda n: n, True)), _eval_fastmath, f64_only=True),
    "eval_texture": Hook(dict(rgb=("R", lambda n: 3 * n, False)), _eval_texture),
    "eval_disk_emission_observer": Hook(dict(omega=("R", lambda n: n, True), u_emit=("R", lambda n: 4 * n, True), g=("R", lambda n: n, True),
                                             rgb=("R", lambda n: 3 * n, True)), _eval_emission),
    "make_observer_canvas": Hook(dict(state0=("R", lambda n: N * 8, False)), _make_observer_canvas, frame=True),
    "eval_observer": Hook(dict(frame=("R", lambda n: 16, True), omega=("R", lambda n: 1, True), valid=(np.int32, lambda n: 1, True)), _eval_observer, frame=True),
    "eval_hot_spot": Hook(dict(omega_s=("R", lambda n: 1, True), valid=(np.int32, lambda n: 1, True), j=(np.float64, lambda n: n, False)), _eval_hot_spot),
    "eval_spectrum_line": Hook(dict(axis=(np.float64, lambda n: LINE["nb"], True), bin=(np.int64, lambda n: n, True), val=(np.float64, lambda n: n, True)),
                               _eval_spectrum(LINE)),
    "eval_spectrum_thermal": Hook(dict(axis=(np.float64, lambda n: THERMAL["nb"], True), bin=(np.int64, lambda n: n, True),
                                       val=(np.float64, lambda n: n * THERMAL["nb"], True)), _eval_spectrum(THERMAL)),
    "eval_polarization": Hook(dict(kappa=("R", lambda n: 2 * n, True), f_em=("R", lambda n: 4 * n, True), aux=("R", lambda n: n, True),
                                   delta=("R", lambda n: n, True), q=("R", lambda n: n, True), u=("R", lambda n: n, True), valid=(np.int32, lambda n: n, True)),
                              _eval_polarization),
    "eval_walker_penrose": Hook(dict(kappa=("R", lambda n: 2 * n, False)), _eval_walker_penrose),
    "trace_polarized": Hook(dict(rgb=("R", lambda n: 3 * N, False), g=("R", lambda n: N, False), q=("R", lambda n: N, False), u=("R", lambda n: N, False),
                                 aux=("R", lambda n: N, True)), _trace_polarized, frame=True),
    "trace_orders": Hook({k: (d, (lambda f: lambda n: f(N))(f), o) for k, (d, f, o) in ORDER_PLANES.items()}, _trace_orders(False), frame=True),
    "trace_orders_state0": Hook({k: (d, (lambda f: lambda n: f(N))(f), o) for k, (d, f, o) in ORDER_PLANES.items()}, _trace_orders(True), frame=True),
}
CASES = [(name, dt) for name, h in HOOKS.items() for dt in DTYPES if not (h.f64_only and dt is np.float32)]
IDS = [f"{name}-{np.dtype(dt).name}" for name, dt in CASES]


def run(lib, name, dtype, n, omit=None, keep_count=False):
    """one call: every output an Out sized for n points (keep_count: for N, whatever n is), `omit` passed as NULL -> (status, {name: Out})"""
    h = HOOKS[name]
    suf = "f64" if dtype == np.float64 else "f32"
    outs = {k: Out(dtype if d == "R" else d, cnt(N if keep_count else n)) for k, (d, cnt, _) in h.outputs.items()}
    p = {k: (None if k == omit else o.ptr) for k, o in outs.items()}
    rc = h.call(lib, suf, points(lib, dtype), n, p)
    return rc, outs


_FULL = {}


def full(lib, name, dtype):
    key = (name, np.dtype(dtype).name)
    if key not in _FULL:
        _FULL[key] = run(lib, name, dtype, N)
    return _FULL[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", CASES, ids=IDS)
def test_guard_words_stay_and_every_element_is_written(lib, name, dtype):
    """(a) every output 64 bytes longer than needed and full of a byte pattern: the 64 bytes are intact after the call (no copy too long), and no
    whole element of the array still holds the pattern (no copy too short or left out) — compared as bits, so that a NaN result counts as
    written."""
    rc, outs = full(lib, name, dtype)
    abi.check(lib, rc)
    for k, o in outs.items():
        assert o.guard_intact(), f"{name}: bytes behind `{k}` were written"
        assert o.elements_left() == 0, f"{name}: {o.elements_left()} of {o.count} elements of `{k}` were not written"


OMIT = [(name, dt, k) for name, dt in CASES for k, (_, _, optional) in HOOKS[name].outputs.items() if optional]


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype,omit", OMIT, ids=[f"{n}-{np.dtype(d).name}-{k}" for n, d, k in OMIT])
def test_an_omitted_output_changes_no_other(lib, name, dtype, omit):
    """(b) each optional output NULL in turn: the call succeeds, and every other output is bitwise what the call with all outputs gives."""
    _, want = full(lib, name, dtype)
    rc, got = run(lib, name, dtype, N, omit=omit)
    abi.check(lib, rc)
    for k, o in got.items():
        if k != omit:
            assert o.guard_intact() and o.bits() == want[k].bits(), f"{name} without `{omit}`: `{k}` differs"


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", [c for c in CASES if not HOOKS[c[0]].frame], ids=[i for c, i in zip(CASES, IDS) if not HOOKS[c[0]].frame])
def test_no_points_is_ok_and_touches_nothing(lib, name, dtype):
    """(c) n = 0 with every array in place: RTGR_OK, and no byte of any array changes.  (rtgr_eval_hot_spot_*'s omega_s and valid, and
    rtgr_eval_spectrum_*'s axis, do not depend on the points: they are answered for n = 0 too, and are the exception.)"""
    rc, outs = run(lib, name, dtype, 0, keep_count=True)
    assert rc == abi.OK, lib.rtgr_last_error()
    answered = {"eval_hot_spot": ("omega_s", "valid"), "eval_spectrum_line": ("axis",), "eval_spectrum_thermal": ("axis",)}.get(name, ())
    for k, o in outs.items():
        if k in answered:
            assert o.guard_intact() and o.elements_left() == 0, f"{name}: `{k}` is answered without points too"
        else:
            assert o.untouched(), f"{name}: `{k}` was written by a call with n = 0"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
def test_eval_texture_keeps_the_entry_of_a_point_with_no_sample(lib, dtype):
    """(d) rgb goes up as well as down: a zero direction is "no sample" and keeps the caller's entry — in the middle of the first block, and
    as the one point of the second — while its neighbours are overwritten."""
    suf = "f64" if dtype == np.float64 else "f32"
    d = points(lib, dtype)["dir"].copy()
    holes = (100, N - 1)
    for k in holes:
        d[k] = 0
    rgb = np.full((N, 3), -7.0, dtype)
    rgb[:, 1] = -np.arange(1, N + 1)
    before = rgb.copy()
    abi.check(lib, getattr(lib, "rtgr_eval_texture_" + suf)(None, texture(lib), abi.TEX_BILINEAR, d.ctypes.data, N, None, rgb.ctypes.data))
    for k in range(N):
        if k in holes:
            assert rgb[k].tobytes() == before[k].tobytes(), k
        else:
            assert (rgb[k] >= 0).all() and (rgb[k] <= 1).all(), (k, rgb[k])   # a texel of [0.1, 0.9], none of the negative entries
