"""The observer camera in the Julia stub (julia/RayTraceGRHIP.jl: RtgrObserver, Observer, trace_rays_observer), cross-checked statically —
no Julia runtime — against include/rtgr.h and the ctypes mirror, with the helpers of tests/test_julia_stub.py (which also holds every
ccall of the stub, these two included, against its C prototype)."""
import ctypes
import re

from test_julia_stub import HDR, JL, abi, c_kind, c_prototypes, ccalls, jl_kind, strip_julia


def test_the_julia_stub_binds_the_observer_camera():
    text = open(JL).read()
    code = strip_julia(text)
    hdr = re.sub(r"/\*(?:.|\n)*?\*/", " ", open(HDR).read())
    # the struct: field names and order as in the header, the fieldoffset table as the ctypes mirror lays it out
    body = re.search(r"struct RtgrObserver[ \t]*\n((?:.|\n)*?)\nend", code).group(1)
    jfields = re.findall(r"([A-Za-z_0-9]+)::", body)
    cbody = re.search(r"typedef struct[^{]*\{((?:[^{}]|\{[^{}]*\})*)\}\s*rtgr_observer\s*;", hdr).group(1)
    cfields = []
    for d in cbody.split(";"):
        if d.strip():
            names = d.strip().split(None, 1)[1]                      # `double look[4], up[4]` declares two
            cfields += [re.sub(r"\[.*", "", n.strip()) for n in names.split(",")]
    assert jfields == cfields == [n for n, _ in abi.rtgr_observer._fields_], (jfields, cfields)
    m = re.search(r"^#\s+RtgrObserver\s+(\d+)\s+(.*)$", text, re.M)
    assert m and int(m.group(1)) == ctypes.sizeof(abi.rtgr_observer) == 176
    fields = [(n, int(o)) for n, o in re.findall(r"([a-z_A-Z0-9]+) (\d+)", m.group(2))]
    assert fields == [(n, getattr(abi.rtgr_observer, n).offset) for n, _ in abi.rtgr_observer._fields_], fields
    # the constants
    cvals = {k: int(v) for k, v in re.findall(r"\b(RTGR_(?:OBS|PROJ)_[A-Z]+)\s*=\s*(\d+)", hdr)}
    jvals = {k: int(v) for k, v in re.findall(r"const\s+(RTGR_(?:OBS|PROJ)_[A-Z]+)\s*=\s*UInt32\((\d+)\)", code)}
    assert jvals == cvals and len(cvals) == 5, (jvals, cvals)
    # the entry points: both scalar types, argument for argument
    protos = c_prototypes()
    bound = {c[0]: c for c in ccalls() if "observer" in c[0]}
    assert set(bound) == {"rtgr_trace_observer_f64", "rtgr_trace_observer_f32", "rtgr_eval_observer_f64", "rtgr_eval_observer_f32"}
    for sym, (_, ret, types, args) in bound.items():
        cret, cparams = protos[sym]
        assert ret == "Cint" and cret == "int" and len(types) == len(args) == len(cparams) == (12 if "trace" in sym else 6)
        assert [jl_kind(t) for t in types] == [c_kind(t) for t in cparams]
        at = 3 if "trace" in sym else 2
        assert types[at].strip() == "Ptr{RtgrObserver}" and "rtgr_observer" in cparams[at]
    for sym in ("rtgr_eval_observer_f64", "rtgr_eval_observer_f32"):
        assert bound[sym][2][-1].strip() == "Ptr{Cint}" and "int*" in protos[sym][1][-1].replace(" *", "*")
    for word in ("function trace_rays_observer(", "function Observer(", "function observer_frame("):
        assert word in text, word
    # the mirror asks the hook first and raises: the call of observer_frame precedes the trace's ccall, and observer_frame errors on valid == 0
    body = code[code.index("function trace_rays_observer("):]
    body = body[:body.index("\nend\n")]
    assert 0 < body.index("observer_frame(scene, obs") < body.index("ccall(")
    hook = code[code.index("function observer_frame("):]
    hook = hook[:hook.index("\nend\n")]
    assert re.search(r"valid\[\]\s*==\s*0\s*&&\s*error\(", hook), hook
