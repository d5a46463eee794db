// rtgr_grid_interp.hpp — metrics given as SAMPLES (RTGR_GRID, include/rtgr.h; the time-dependent RTGR_GRID4, rtgr_args.hpp): the
// interpolant, and the one seam through which the rest of the device code meets a sampled metric — the trait Sampled<R, METRIC> where
// the metric is known at compile time (the integrate / prepare kernels), sampled_metric<R, NE> / sampled_accel<R, NE> behind
// sampled_on(sc.metric, NE) where it is read at run time (the hooks of rtgr_misc.hip).  A new kind is a row loop here, a case of
// sampled_eval and one of sampled_dims (rtgr_args.hpp).  Included by rtgr_physics.hpp, behind the generic contraction it feeds.
#pragma once
namespace rtgr {
// ---- one axis -------------------------------------------------------------------------------------------------------------------
// Tricubic Catmull-Rom (cubic convolution, a = −1/2), separable.  Per axis: s = (x − origin)/h, i = clamp(floor(s), 1, n − 3),
// t = s − i, weights on samples i−1 … i+2 and their t-derivatives (× 1/h).  The clamp is written with comparisons that are false for
// NaN, so a non-finite coordinate still reads samples inside the table (its value is then NaN, and so is the ray: RTGR_RAY_NAN).
// An axis is named by what holds its descriptor and its index there: (DevGrid, 0..2) for x, y, z, (DevGridTime, ·) for t.
template <class R> RTGR_DEV R axis_origin(const DevGrid<R>& G, int ax) { return G.origin[ax]; }
template <class R> RTGR_DEV R axis_inv_h(const DevGrid<R>& G, int ax) { return G.inv_h[ax]; }
template <class R> RTGR_DEV R axis_hi(const DevGrid<R>& G, int ax) { return G.hi[ax]; }
template <class R> RTGR_DEV R axis_origin(const DevGridTime<R>& T, int) { return T.origin; }
template <class R> RTGR_DEV R axis_inv_h(const DevGridTime<R>& T, int) { return T.inv_h; }
template <class R> RTGR_DEV R axis_hi(const DevGridTime<R>& T, int) { return T.hi; }
// the cell of coordinate x on an axis: returns the stencil's first sample, t = s − i
template <class R, class A> RTGR_DEV uint64_t grid_cell(const A& G, int ax, R x, R& t) {
    const R s = (x - axis_origin<R>(G, ax)) * axis_inv_h<R>(G, ax);
    R c = rfloor(s);
    c = c > axis_hi<R>(G, ax) ? axis_hi<R>(G, ax) : c;
    c = c >= R(1) ? c : R(1);
    t = s - c;
    return (uint64_t)c - 1u;                                      // first sample of the stencil
}
// The weights on samples i−1 … i+2 and their derivatives × 1/h, from t and 1/h.  The polynomials stand twice, here and nowhere else:
// for all four and for weight k alone (below).  Folding the first into four calls of the second computes the same values but moves the
// compiler's schedule in EVERY unit (each one's camera carries grid_eval); those are held byte for byte (profiles/grid/refactor_isa.md).
template <class R> RTGR_DEV void grid_weights(R t, R inv_h, R w[4], R dw[4]) {
    const R t2 = t * t, t3 = t2 * t, ih = R(0.5) * inv_h;
    w[0] = R(0.5) * rfma(R(2), t2, -t3 - t);                      // (−t³ + 2t² − t)/2
    w[1] = R(0.5) * rfma(R(3), t3, rfma(R(-5), t2, R(2)));        // (3t³ − 5t² + 2)/2
    w[2] = R(0.5) * rfma(R(-3), t3, rfma(R(4), t2, t));           // (−3t³ + 4t² + t)/2
    w[3] = R(0.5) * (t3 - t2);                                    // (t³ − t²)/2
    dw[0] = ih * rfma(R(-3), t2, rfma(R(4), t, R(-1)));           // (−3t² + 4t − 1)/2h
    dw[1] = ih * rfma(R(9), t2, R(-10) * t);                      // (9t² − 10t)/2h
    dw[2] = ih * rfma(R(-9), t2, rfma(R(8), t, R(1)));            // (−9t² + 8t + 1)/2h
    dw[3] = ih * rfma(R(3), t2, R(-2) * t);                       // (3t² − 2t)/2h
}
// weight k (0..3) and its derivative alone; k is wave-uniform where it is used (the row loop's counter)
template <class R> RTGR_DEV void grid_weight(int k, R t, R ih, R& w, R& dw) {
    const R t2 = t * t, t3 = t2 * t;
    ih = R(0.5) * ih;
    if (k == 0) { w = R(0.5) * rfma(R(2), t2, -t3 - t); dw = ih * rfma(R(-3), t2, rfma(R(4), t, R(-1))); }
    else if (k == 1) { w = R(0.5) * rfma(R(3), t3, rfma(R(-5), t2, R(2))); dw = ih * rfma(R(9), t2, R(-10) * t); }
    else if (k == 2) { w = R(0.5) * rfma(R(-3), t3, rfma(R(4), t2, t)); dw = ih * rfma(R(-9), t2, rfma(R(8), t, R(1))); }
    else { w = R(0.5) * (t3 - t2); dw = ih * rfma(R(3), t2, R(-2) * t); }
}
// cell and weights of an axis whose weights are kept for the whole stencil (x; t of a 4-D grid)
template <class R, class A> RTGR_DEV uint64_t grid_axis(const A& G, int ax, R x, R w[4], R dw[4]) {
    R t;
    const uint64_t i = grid_cell<R>(G, ax, x, t);
    grid_weights<R>(t, axis_inv_h<R>(G, ax), w, dw);
    return i;
}
// ---- the row loops: one per kind (their register and bytes-in-flight shapes were tuned separately) ---------
// g (the 10 components of the upper triangle, tt tx ty tz xx xy xz yy yz zz) and ∂_x g, ∂_y g, ∂_z g at a spatial point.  The stencil
// is 16 rows of 4 consecutive x-samples (40 contiguous scalars each, the caller's layout), walked row by row (a loop, not unrolled: the
// 640 loads of a fully unrolled stencil were hoisted ahead of the arithmetic, ~5 KB of spills per lane); per row the x-weights are combined first, then the
// row's y·z weights.  Everything is summed RELATIVE to the stencil's centre sample s₁₁₁: g = s₁₁₁ + Σ W (s − s₁₁₁), ∂g = Σ W' (s − s₁₁₁)
// — the same polynomials (Σ W = 1, Σ W' = 0), and exact where the samples are constant: a flat stretch of the table gives g to the bit
// and ∂g = 0 exactly, not a few ulp of rounding through weights that sum to 1 − ε.
template <class R> RTGR_DEV void grid_eval(const DevGrid<R>& G, const R xs[3], R v[10], R d[3][10]) {
    R wx[4], dwx[4], ty, tz;   // (the y and z weights are formed per row from t: 16 fewer live registers)
    const uint64_t ix = grid_axis<R>(G, 0, xs[0], wx, dwx);
    const uint64_t iy = grid_cell<R>(G, 1, xs[1], ty);
    const uint64_t iz = grid_cell<R>(G, 2, xs[2], tz);
    const R* base = G.g + iz * G.sz + iy * G.sy + ix * 10u;
    R ref[10];
    const R* centre = base + G.sz + G.sy + 10u;
#pragma unroll
    for (int c = 0; c < 10; c++) { ref[c] = centre[c]; v[c] = R(0); d[0][c] = R(0); d[1][c] = R(0); d[2][c] = R(0); }
#pragma unroll 1
    for (int r = 0; r < 16; r++) {
        const int ky = r & 3, kz = r >> 2;
        R wyk, dwyk, wzk, dwzk;
        grid_weight<R>(ky, ty, G.inv_h[1], wyk, dwyk);
        grid_weight<R>(kz, tz, G.inv_h[2], wzk, dwzk);
        const R wv = wyk * wzk, wdy = dwyk * wzk, wdz = wyk * dwzk;
        const R* row = base + (uint64_t)kz * G.sz + (uint64_t)ky * G.sy;
#pragma unroll
        for (int c = 0; c < 10; c++) {
            const R a0 = row[c] - ref[c], a1 = row[10 + c] - ref[c], a2 = row[20 + c] - ref[c], a3 = row[30 + c] - ref[c];
            const R rv = rfma(wx[3], a3, rfma(wx[2], a2, rfma(wx[1], a1, wx[0] * a0)));
            const R rd = rfma(dwx[3], a3, rfma(dwx[2], a2, rfma(dwx[1], a1, dwx[0] * a0)));
            v[c] = rfma(wv, rv, v[c]);
            d[0][c] = rfma(wv, rd, d[0][c]);
            d[1][c] = rfma(wdy, rv, d[1][c]);
            d[2][c] = rfma(wdz, rv, d[2][c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 10; c++) v[c] = v[c] + ref[c];
}
// A time-dependent grid (rtgr_grid4_metric_load): the tensor product of the same weights on t, x, y, z.
// g (upper triangle) and d[0] = ∂_t g, d[1..3] = ∂_x,y,z g at (xt, xs).  The stencil is 4 slices x the 16 spatial rows of grid_eval,
// walked as grid_eval walks them: 16 trips, each loading the four slices' copies of one row together (160 scalars, 4x the bytes in
// flight of a 3-D trip).  Per row the slices are blended FIRST, relative to the time-centre slice s₁:
//     b = (s₁ − ref) + Σ_l w_t,l (s_l − s₁),    b' = Σ_l w'_t,l (s_l − s₁)        (l = 0, 2, 3: the l = 1 term is exactly 0)
// with ref the centre sample of the centre slice; b then goes through grid_eval's x-weights / y·z-weights exactly, and b' through
// the same x- and y·z-weights into ∂_t g.  A grid whose slices are all equal therefore gives b = s₁ − ref, i.e. g and ∂_x,y,z g
// bit for bit as grid_eval on one slice, and ∂_t g = 0 exactly.
template <class R> RTGR_DEV void grid4_eval(const DevGrid<R>& G, const DevGridTime<R>& T, R xt, const R xs[3], R v[10], R d[4][10]) {
    R wx[4], dwx[4], ty, tz, wt[4], dwt[4];
    const uint64_t ix = grid_axis<R>(G, 0, xs[0], wx, dwx);
    const uint64_t iy = grid_cell<R>(G, 1, xs[1], ty);
    const uint64_t iz = grid_cell<R>(G, 2, xs[2], tz);
    const uint64_t it = grid_axis<R>(T, 0, xt, wt, dwt);
    const uint64_t st = T.st;
    const R* base = G.g + it * st + iz * G.sz + iy * G.sy + ix * 10u;   // slice 0 of the stencil; slice l is l·st further
    R ref[10];
    const R* centre = base + st + G.sz + G.sy + 10u;
#pragma unroll
    for (int c = 0; c < 10; c++) {
        ref[c] = centre[c];
        v[c] = R(0);
#pragma unroll
        for (int j = 0; j < 4; j++) d[j][c] = R(0);
    }
#pragma unroll 1
    for (int r = 0; r < 16; r++) {
        const int ky = r & 3, kz = r >> 2;
        R wyk, dwyk, wzk, dwzk;
        grid_weight<R>(ky, ty, G.inv_h[1], wyk, dwyk);
        grid_weight<R>(kz, tz, G.inv_h[2], wzk, dwzk);
        const R wv = wyk * wzk, wdy = dwyk * wzk, wdz = wyk * dwzk;
        const R* row = base + (uint64_t)kz * G.sz + (uint64_t)ky * G.sy;
#pragma unroll
        for (int c = 0; c < 10; c++) {
            R b[4], bt[4];
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const R s1 = row[st + 10 * m + c];
                const R e0 = row[10 * m + c] - s1, e2 = row[2 * st + 10 * m + c] - s1, e3 = row[3 * st + 10 * m + c] - s1;
                b[m] = (s1 - ref[c]) + rfma(wt[3], e3, rfma(wt[2], e2, wt[0] * e0));
                bt[m] = rfma(dwt[3], e3, rfma(dwt[2], e2, dwt[0] * e0));
            }
            const R rv = rfma(wx[3], b[3], rfma(wx[2], b[2], rfma(wx[1], b[1], wx[0] * b[0])));
            const R rd = rfma(dwx[3], b[3], rfma(dwx[2], b[2], rfma(dwx[1], b[1], dwx[0] * b[0])));
            const R rt = rfma(wx[3], bt[3], rfma(wx[2], bt[2], rfma(wx[1], bt[1], wx[0] * bt[0])));
            v[c] = rfma(wv, rv, v[c]);
            d[0][c] = rfma(wv, rt, d[0][c]);
            d[1][c] = rfma(wv, rd, d[1][c]);
            d[2][c] = rfma(wdy, rv, d[2][c]);
            d[3][c] = rfma(wdz, rv, d[3][c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 10; c++) v[c] = v[c] + ref[c];
}
// ---- what every kind shares, by the number NE of coordinates it depends on (3: x, y, z; 4: t too) --------------------------------
// the time axis' descriptor of a 4-D grid: GRID4_HEADER bytes in front of the samples (rtgr_args.hpp), one wave-uniform read
template <class R> RTGR_DEV DevGridTime<R> grid4_time(const DevGrid<R>& G) { return *(const DevGridTime<R>*)((const char*)G.g - GRID4_HEADER); }
// g (upper triangle) and its NE partials d[0 .. NE−1] = ∂_(4−NE) … ∂_z g: the row loop of the kind (T, xt: read when NE = 4 only)
template <class R, int NE> RTGR_DEV void sampled_eval(const DevGrid<R>& G, const DevGridTime<R>& T, R xt, const R xs[3], R v[10], R d[NE][10]) {
    if constexpr (NE == 4) grid4_eval<R>(G, T, xt, xs, v, d);
    else grid_eval<R>(G, xs, v, d);
}
// inside the valid box: s in [1, n − 2] on every axis the kind has (false for NaN)
template <class R, int NE> RTGR_DEV bool sampled_inside(const DevGrid<R>& G, const DevGridTime<R>& T, const R x[4]) {
    bool in = true;
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        const R s = (x[1 + ax] - G.origin[ax]) * G.inv_h[ax];
        in = in && s >= R(1) && s <= G.top[ax];
    }
    if constexpr (NE == 4) {
        const R s = (x[0] - T.origin) * T.inv_h;
        in = in && s >= R(1) && s <= T.top;
    }
    return in;
}
// index of component (p, q), p <= q, in the 10-vector
RTGR_DEV constexpr int grid_comp(int p, int q) { return p == 0 ? q : (p == 1 ? 3 + q : (p == 2 ? 5 + q : 9)); }
// the geodesic acceleration of a sampled metric: the interpolant's g and ∂_j g into the generic contraction (NE = 3: stationary)
template <class R, int NE> RTGR_DEV void sampled_accel(const DevGrid<R>& G, const DevGridTime<R>& T, R xt, const R xs[3], const R u[4], R ud[4]) {
    R v[10], d[NE][10];
    sampled_eval<R, NE>(G, T, xt, xs, v, d);
    DDual<R, NE, true> gd[4][4];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = p; q < 4; q++) {
            const int c = grid_comp(p, q);
            gd[p][q].v = v[c];
#pragma unroll
            for (int j = 0; j < NE; j++) gd[p][q].e[j] = d[j][c];
        }
    generic_contract<R, NE, true>(gd, u, ud);
}
// g and dg[a][b][c] = ∂_c g_ab (∂_t = 0 when NE = 3) at a 4-position: rtgr_eval_metric_*, make_canvas, redshift
template <class R, int NE> RTGR_DEV void sampled_metric(const DevGrid<R>& G, const R x[4], R g[4][4], R dg[4][4][4]) {
    R v[10], d[NE][10];
    DevGridTime<R> T{};
    if constexpr (NE == 4) T = grid4_time<R>(G);
    sampled_eval<R, NE>(G, T, x[0], x + 1, v, d);
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = p <= q ? grid_comp(p, q) : grid_comp(q, p);
            g[p][q] = v[c];
            if constexpr (NE == 3) dg[p][q][0] = R(0);
#pragma unroll
            for (int j = 0; j < NE; j++) dg[p][q][4 - NE + j] = d[j][c];
        }
}
// ---- the seam: what an instantiation on METRIC needs to know about sampled metrics.  For every other METRIC `is` is false, fill does
// nothing and the rest is never called (the constants do not depend on R: Sampled<double, METRIC> where there is no scalar type) ------
template <class R, int METRIC>
struct Sampled {
    static constexpr int dims = METRIC >= RTGR_GENERIC_BASE ? sampled_dims((uint32_t)(METRIC - RTGR_GENERIC_BASE)) : 0;
    static constexpr bool is = dims != 0, time_dependent = dims == 4;
    static constexpr int NE = time_dependent ? 4 : 3;   // coordinates the metric depends on = partials the RHS carries
    // the grid's descriptor into the wave-uniform constants of the instantiation (scene_consts)
    static RTGR_DEV void fill(MetricK<R>& k, const DevScene<R>& sc) {
        if constexpr (is) k.grid = sc.grid;
        if constexpr (time_dependent) {
            k.gt = grid4_time<R>(sc.grid);
            k.gt.origin = uniform_(k.gt.origin); k.gt.inv_h = uniform_(k.gt.inv_h); k.gt.hi = uniform_(k.gt.hi); k.gt.top = uniform_(k.gt.top);
            k.gt.st = uniform64(k.gt.st);
        }
    }
    static RTGR_DEV bool inside(const MetricK<R>& k, const R x[4]) { return sampled_inside<R, NE>(k.grid, k.gt, x); }
    static RTGR_DEV void accel(const MetricK<R>& k, R xt, const R xs[3], const R u[4], R ud[4]) { sampled_accel<R, NE>(k.grid, k.gt, xt, xs, u, ud); }
};
}  // namespace rtgr
