// rtgr_grid.hip — metrics sampled on a grid (RTGR_GRID, include/rtgr.h; 3-D and time-dependent 4-D): the checks of a load and the images it
// uploads, in Float64 and Float32, and the unload — both through the one path of rtgr_tables.hip (retire: a hipGraph captured earlier may
// still replay the samples; rtgr_trim frees them).  Host code only: the interpolant is rtgr_grid_interp.hpp's (grid_eval, grid4_eval), the kernels are tu_f64_grid.hip's / tu_f32_grid.hip's and
// tu_f64_grid4.hip's / tu_f32_grid4.hip's; what the kernels read of the axes is built from GridAxes in rtgr_host.hpp (dev_grid, dev_grid_time).
#include <cmath>
#include "rtgr_internal.hpp"

namespace rtgr {

// Grid ids: a counter of their own, in a range of their own (top bits 0xA...), and never the id of a resident unit or table of the
// context (table_load).
constexpr uint64_t GRID_ID_TAG = 0xA000000000000000ull;
static TableIds g_grid_ids{GRID_ID_TAG, GRID_ID_TAG};

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

// The load of either kind.  Checks the axes and every sample, then has Float64 and Float32 copies uploaded to every device (a 4-D table
// behind the GRID4_HEADER bytes of its time axis' descriptor, rtgr_args.hpp) and the table published under a fresh id (table_load).
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
    // a 4-D table starts with the GRID4_HEADER bytes of its time axis' descriptor (DevGridTime, read by the kernels), in each scalar type
    const DevGridTime<double> t64 = dev_grid_time<double>(A);
    const DevGridTime<float> t32 = dev_grid_time<float>(A);
    static_assert(sizeof(DevGridTime<double>) <= GRID4_HEADER && sizeof(DevGridTime<float>) <= GRID4_HEADER, "GRID4_HEADER");
    char head64[GRID4_HEADER] = {}, head32[GRID4_HEADER] = {};
    std::memcpy(head64, &t64, sizeof t64);
    std::memcpy(head32, &t32, sizeof t32);
    GridTable t;
    t.axes = A;
    TableImage image64, image32;
    if (nt) { image64.push_back({head64, sizeof head64}); image32.push_back({head32, sizeof head32}); }
    image64.push_back({g, (size_t)npts * 10 * sizeof(double)});
    image32.push_back({g32.data(), (size_t)npts * 10 * sizeof(float)});
    return table_load(c, who, g_grid_ids, &DeviceCtx::grids, t, image64, image32, id_out);
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
    const bool found = table_unload(c, &DeviceCtx::grids, id, false);   // (id 0 names no grid)
    if (!found) return fail(RTGR_ERR_BAD_ARG, "rtgr_grid_metric_unload: no grid metric with id " + std::to_string(id) + " is loaded in this context");
    return RTGR_OK;
}

}  // namespace rtgr
