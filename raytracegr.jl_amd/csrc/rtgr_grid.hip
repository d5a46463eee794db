// rtgr_grid.hip — metrics sampled on a grid (RTGR_GRID, include/rtgr.h; 3-D and time-dependent 4-D): load (checks, upload to every device of the context in
// Float64 and Float32) and unload (retire: a hipGraph captured earlier may still replay the samples; rtgr_trim frees them).  Host code
// only: the interpolant is rtgr_grid_interp.hpp's (grid_eval, grid4_eval), the kernels are tu_f64_grid.hip's / tu_f32_grid.hip's and
// tu_f64_grid4.hip's / tu_f32_grid4.hip's; what the kernels read of the axes is built from GridAxes in rtgr_host.hpp (dev_grid, dev_grid_time).
#include <atomic>
#include <cmath>
#include "rtgr_internal.hpp"

namespace rtgr {

// Grid ids: a counter of their own, in a range of their own (top bits 0xA...), and never the id of a resident unit of the context.
static std::atomic<uint64_t> g_next_grid{1};
constexpr uint64_t GRID_ID_TAG = 0xA000000000000000ull;

// det of the symmetric 4x4 given by its upper triangle tt tx ty tz xx xy xz yy yz zz (long double: a Lorentzian sample near
// degenerate must not be refused for rounding)
static long double det_upper(const double* c) {
    const long double m00 = c[0], m01 = c[1], m02 = c[2], m03 = c[3], m11 = c[4], m12 = c[5], m13 = c[6], m22 = c[7], m23 = c[8], m33 = c[9];
    const long double s0 = m00 * m11 - m01 * m01, s1 = m00 * m12 - m01 * m02, s2 = m00 * m13 - m01 * m03;
    const long double s3 = m01 * m12 - m11 * m02, s4 = m01 * m13 - m11 * m03, s5 = m02 * m13 - m12 * m03;
    const long double c0 = m02 * m13 - m03 * m12, c1 = m02 * m23 - m03 * m22, c2 = m02 * m33 - m03 * m23;
    const long double c3 = m12 * m23 - m13 * m22, c4 = m12 * m33 - m13 * m23, c5 = m22 * m33 - m23 * m23;
    return s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
}

// The load of either kind.  Checks the axes and every sample, then uploads Float64 and Float32 copies to every device (a 4-D table
// behind the GRID4_HEADER bytes of its time axis' descriptor, rtgr_args.hpp) and publishes the table under a fresh id.
static int grid_load(rtgr_context* c, const char* who, const GridAxes& A, const double* g, uint64_t* id_out) {
    const bool nt = A.dims == 4;
    const uint32_t* n = A.n + 1;   // the spatial axes
    uint64_t npts = 1;
    for (int k = 0; k < A.dims; k++) {
        const int ax = k < 3 ? k + 1 : 0;   // x, y, z, then t
        const uint32_t na = A.n[ax];
        const double o = A.origin[ax], h = A.spacing[ax];
        const std::string name = std::to_string(nt ? ax : ax - 1);   // (the caller's numbering: t, x, y, z of rtgr_grid4; x, y, z of rtgr_grid)
        if (na < 4u || na > (1u << 20))
            return fail(RTGR_ERR_BAD_ARG, std::string(who) + ": n[" + name + "] = " + std::to_string(na) + ": each axis needs 4 .. 2^20 samples");
        if (!(h > 0.0) || !std::isfinite(h) || !std::isfinite(o))
            return fail(RTGR_ERR_BAD_ARG, std::string(who) + ": spacing must be finite and > 0, origin finite (axis " + name + ")");
        if (npts <= RTGR_GRID_MAX_SAMPLES) npts *= na;   // (stops growing past the cap: <= 2^28 x 2^20, no uint64_t overflow on four axes)
    }
    if (npts > RTGR_GRID_MAX_SAMPLES)
        return fail(RTGR_ERR_BAD_ARG, std::string(who) + ": " + std::to_string(npts) + " samples, more than RTGR_GRID_MAX_SAMPLES");
    // every sample finite and Lorentzian-signed (det g < 0; a transposed layout fails this at once), and the Float32 copy
    std::vector<float> g32((size_t)npts * 10);
    for (uint64_t p = 0; p < npts; p++) {
        const double* v = g + p * 10;
        bool finite = true;
        for (int k = 0; k < 10; k++) { finite = finite && std::isfinite(v[k]); g32[p * 10 + k] = (float)v[k]; }
        if (!finite || !(det_upper(v) < 0.0L)) {
            const uint64_t i = p % n[0], j = (p / n[0]) % n[1], k = (p / ((uint64_t)n[0] * n[1])) % n[2];
            const uint64_t l = p / ((uint64_t)n[0] * n[1] * n[2]);
            return fail(RTGR_ERR_BAD_ARG, std::string(who) + ": sample " + std::to_string(p) +
                                          (nt ? " (l, k, j, i) = (" + std::to_string(l) + ", " : std::string(" (i, j, k) = (")) +
                                          (nt ? std::to_string(k) + ", " + std::to_string(j) + ", " + std::to_string(i)
                                              : std::to_string(i) + ", " + std::to_string(j) + ", " + std::to_string(k)) + ") " +
                                          (finite ? (nt ? "has det g >= 0 (not a Lorentzian metric: components in the order tt tx ty tz xx xy xz yy yz zz, x fastest, t slowest?)"
                                                        : "has det g >= 0 (not a Lorentzian metric: components in the order tt tx ty tz xx xy xz yy yz zz, x fastest?)")
                                                  : "holds a non-finite value"));
        }
    }
    // a 4-D table starts with its time axis' descriptor (DevGridTime, read by the kernels), in each scalar type
    const size_t head = nt ? (size_t)GRID4_HEADER : 0;
    const DevGridTime<double> t64 = dev_grid_time<double>(A);
    const DevGridTime<float> t32 = dev_grid_time<float>(A);
    static_assert(sizeof(DevGridTime<double>) <= GRID4_HEADER && sizeof(DevGridTime<float>) <= GRID4_HEADER, "GRID4_HEADER");
    const size_t b64 = (size_t)npts * 10 * sizeof(double), b32 = (size_t)npts * 10 * sizeof(float);
    std::lock_guard<std::mutex> load_lock(c->modules_mu);   // (units and grids are loaded / unloaded under the same lock)
    uint64_t id = 0;
    for (;;) {
        id = GRID_ID_TAG | (g_next_grid.fetch_add(1) & ~GRID_ID_TAG);
        bool taken = false;
        for (auto& d : c->devs) {
            std::lock_guard<std::mutex> lk(d->mu);
            taken = taken || d->find_module(id) || d->find_grid(id);
        }
        if (!taken) break;
    }
    // allocate and upload everywhere first; the tables become visible to scenes only when every device has its copy
    std::vector<GridTable> made(c->devs.size());
    auto release = [&]() {
        for (size_t k = 0; k < made.size(); k++) {
            DeviceGuard guard(c->devs[k]->dev);
            if (made[k].d64) (void)hipFree(made[k].d64);
            if (made[k].d32) (void)hipFree(made[k].d32);
        }
    };
    for (size_t k = 0; k < c->devs.size(); k++) {
        DeviceGuard guard(c->devs[k]->dev);
        if (!guard.ok) { release(); return fail(RTGR_ERR_HIP, "hipSetDevice failed"); }
        GridTable& t = made[k];
        t.id = id;
        t.axes = A;
        hipError_t e = hipMalloc(&t.d64, head + b64);
        if (e == hipSuccess) e = hipMalloc(&t.d32, head + b32);
        if (e == hipSuccess && nt) e = hipMemcpy(t.d64, &t64, sizeof t64, hipMemcpyHostToDevice);
        if (e == hipSuccess && nt) e = hipMemcpy(t.d32, &t32, sizeof t32, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy((char*)t.d64 + head, g, b64, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy((char*)t.d32 + head, g32.data(), b32, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            release();
            return fail(RTGR_ERR_HIP, std::string(who) + ": upload to device " + std::to_string(k) + ": " + hipGetErrorString(e));
        }
    }
    for (size_t k = 0; k < c->devs.size(); k++) {
        std::lock_guard<std::mutex> lk(c->devs[k]->mu);
        c->devs[k]->grids.push_back(made[k]);
    }
    *id_out = id;
    return RTGR_OK;
}

int api::grid_metric_load(rtgr_context* ctx, const rtgr_grid* grid, const double* g, uint64_t* id_out) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if (!grid || !g || !id_out) return fail(RTGR_ERR_BAD_ARG, "rtgr_grid_metric_load: NULL argument");
    if (grid->pad != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_grid_metric_load: rtgr_grid.pad must be 0");
    GridAxes A;
    for (int ax = 0; ax < 3; ax++) { A.n[1 + ax] = grid->n[ax]; A.origin[1 + ax] = grid->origin[ax]; A.spacing[1 + ax] = grid->spacing[ax]; }
    return grid_load(c, "rtgr_grid_metric_load", A, g, id_out);
}

int api::grid4_metric_load(rtgr_context* ctx, const rtgr_grid4* grid, const double* g, uint64_t* id_out) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if (!grid || !g || !id_out) return fail(RTGR_ERR_BAD_ARG, "rtgr_grid4_metric_load: NULL argument");
    GridAxes A;
    A.dims = 4;
    for (int ax = 0; ax < 4; ax++) { A.n[ax] = grid->n[ax]; A.origin[ax] = grid->origin[ax]; A.spacing[ax] = grid->spacing[ax]; }
    return grid_load(c, "rtgr_grid4_metric_load", A, g, id_out);
}

int api::grid_metric_unload(rtgr_context* ctx, uint64_t id) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> load_lock(c->modules_mu);
    bool found = false;
    for (auto& d : c->devs) {
        std::lock_guard<std::mutex> lk(d->mu);
        for (size_t k = 0; k < d->grids.size(); k++)
            if (d->grids[k].id == id) {
                d->retired_grids.push_back(d->grids[k]);   // (not freed: a captured hipGraph may replay it until rtgr_trim)
                d->grids.erase(d->grids.begin() + (long)k);
                found = true;
                break;
            }
    }
    if (!found) return fail(RTGR_ERR_BAD_ARG, "rtgr_grid_metric_unload: no grid metric with id " + std::to_string(id) + " is loaded in this context");
    return RTGR_OK;
}

}  // namespace rtgr

// A test hook, not part of include/rtgr.h (tests/test_grid_metric.py): grid tables on device `index` of the context — resident and
// retired (unloaded, waiting for rtgr_trim).
extern "C" int rtgr_testhook_grid_tables(rtgr_context* ctx, int index, uint32_t* resident, uint32_t* retired) {
    rtgr_context* c = nullptr;
    int rc = rtgr::resolve_ctx(ctx, &c);
    if (rc) return rc;
    if (index < 0 || (size_t)index >= c->devs.size() || !resident || !retired) return rtgr::fail(RTGR_ERR_BAD_ARG, "bad argument");
    rtgr::DeviceCtx& d = *c->devs[(size_t)index];
    std::lock_guard<std::mutex> lk(d.mu);
    *resident = (uint32_t)d.grids.size();
    *retired = (uint32_t)d.retired_grids.size();
    return RTGR_OK;
}
