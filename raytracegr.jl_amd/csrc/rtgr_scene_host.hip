// rtgr_scene_host.hip — argument conversion: the caller's scene, solver and camera into what the kernels read (rtgr_args.hpp); a long
// object list into a device table (object_table, rtgr_tables.hip) with its spheres in groups of neighbours.  Host code only.
#include "rtgr_internal.hpp"

namespace rtgr {

// The band of s whose correctly rounded square root (in R) EQUALS r: lo = min{s : sqrt(s) >= r}, hi = min{s : sqrt(s) > r}.
// disk_sign_distance (rtgr_objects.hpp) reads sign(r − RN(sqrt(s))) off these two thresholds, exactly as the IEEE square root
// of obj_distance would give it.  A few nextafter steps around r² (the root maps 1–3 neighbouring s onto one value).
template <class R>
void disk_sqrt_band(R r, R& lo, R& hi) {
    const R inf = std::numeric_limits<R>::infinity();
    if (!(r >= R(0))) { lo = hi = R(0); return; }      // negative (or NaN) radius: sqrt(s) > r for every s >= 0
    if (r == inf) { lo = hi = inf; return; }
    R c = r * r;
    if (!(c < inf)) c = std::numeric_limits<R>::max();
    for (int it = 0; it < 4096 && c > R(0) && std::sqrt(c) >= r; it++) c = std::nextafter(c, -inf);
    for (int it = 0; it < 4096 && std::sqrt(c) < r; it++) c = std::nextafter(c, inf);
    lo = c;
    for (int it = 0; it < 4096 && std::sqrt(c) <= r; it++) c = std::nextafter(c, inf);
    hi = c;
}

// The (metric enum | generic flag, spin) a scene selects among the kernels' instantiations — what dispatch() below switches on, and
// what a run-time unit without a metric of its own is built for (rtgr_user_unit_desc, rtgr_user_unit.hip.in).
void scene_variant(const rtgr_scene* s, uint32_t* metric, bool* spin) {
    const uint32_t kind = s->metric & ~RTGR_METRIC_GENERIC;
    const bool generic = (s->metric & RTGR_METRIC_GENERIC) != 0 && kind != RTGR_MINKOWSKI;
    *metric = kind | (generic ? RTGR_METRIC_GENERIC : 0u);
    *spin = kind == RTGR_MINKOWSKI ? false : (generic ? true : s->a != 0.0);
}

// What the reach test of every step would otherwise form again from an object's (wave-uniform) parameters: DevObject::nR2 and ::floor_
// (rtgr_args.hpp), from the object AS THE KERNELS SEE IT (the scalar type's values).  THE one place that computes them — every device
// object passes through here: the caller's list (convert_object) and the bounding spheres of its groups (bounding_sphere).
//   nR2    = −R²: it opens the FMA chain of every sphere distance, the scan's included, so it must be the value the kernels' own −R·R
//            has: R·R rounded to nearest in R (the product of two R values is exact in double for Float32, and is the same double
//            multiplication for Float64).
//   floor_ = 2 e R² (1 + 2e) for a sphere, 2 e |p0| (1 + 2e) for a plane (e = reach_eps<R>()), evaluated in double and rounded UP into R
//            — two ulp above the double value, which covers the roundings of the evaluation itself.  What the reach test needs of it is
//            "no smaller than", not tightness.
template <class R>
static void object_constants(DevObject<R>& d) {
    d.nR2 = R(0);
    d.floor_ = R(0);
    if (d.kind != RTGR_SPHERE && d.kind != RTGR_PLANE) return;
    const double e = (double)reach_eps<R>();
    const double r = (double)d.p[8];
    if (d.kind == RTGR_SPHERE) d.nR2 = (R)(-(r * r));
    const double scale = d.kind == RTGR_SPHERE ? r * r : std::fabs((double)d.p[0]);
    double f = 2.0 * e * scale * (1.0 + 2.0 * e);
    f = std::nextafter(std::nextafter(f, HUGE_VAL), HUGE_VAL);
    R fr = (R)f;
    if ((double)fr < f) fr = std::nextafter(fr, std::numeric_limits<R>::infinity());
    d.floor_ = fr;   // (NaN parameters give a NaN floor: the test then never says "out of reach", as before)
}

// one object of the caller's list -> its device form (the scalar type's values; a disk's sign thresholds)
template <class R>
static int convert_object(const rtgr_object& in, DevObject<R>& d) {
    if (in.kind < RTGR_PLANE || in.kind > RTGR_USER_OBJECT)
        return fail(RTGR_ERR_BAD_ARG, "unknown object kind (abstract Object has no distance)");
    d.kind = in.kind;
    d.type = in.kind == RTGR_USER_OBJECT ? in.type : 0u;
    for (int q = 0; q < 9; q++) d.p[q] = (R)in.p[q];
    if (in.kind == RTGR_DISK) {   // p[3..6]: the scan's sign thresholds on x² + y² (device-side only; the ABI's disk is p[0..2])
        disk_sqrt_band<R>(d.p[1], d.p[3], d.p[4]);
        disk_sqrt_band<R>(d.p[2], d.p[5], d.p[6]);
    }
    object_constants<R>(d);
    return RTGR_OK;
}

// ---- groups of a long list's spheres (DevScene, rtgr_args.hpp: GROUPS) ------------------------------------------------------------
struct SphereGroup { uint32_t first, count; };   // positions in the device list
// `order` holds the spheres in the caller's order; on return: [0, *nloose) the spheres that join no group, then the groups' members,
// group by group (`groups`: their positions).  Groups are the leaves of median splits of the centres along the widest axis — a k-d
// tree's leaves, <= RTGR_GROUP_MAX members each (half that for lists of fewer than 36 spheres); a sphere much larger than the list's typical one (a sky sphere around the scene) would
// make its group's bounding sphere as large as itself and stays loose.  Lists with fewer than two full groups, or with a non-finite
// centre or radius among the spheres, get no groups.  Deterministic: ties are broken by the caller's index.
// `supers`: the second level — runs of neighbouring groups (first / count are GROUP indices): the nodes of the same split tree that hold
// at most 8 leaves' worth of spheres; only lists of RTGR_SUPER_FROM groups and more get them.
constexpr size_t RTGR_SUPER_FROM = 24;
static void group_spheres(const rtgr_object* objs, std::vector<uint32_t>& order, uint32_t* nloose, std::vector<SphereGroup>& groups,
                          std::vector<SphereGroup>& supers, size_t leaf = 0, double limit = std::numeric_limits<double>::max()) {
    *nloose = 0;
    groups.clear();
    supers.clear();
    const size_t n = order.size();
    if (n < 2 * (size_t)RTGR_GROUP_MAX) return;
    std::vector<double> radii(n);
    for (size_t k = 0; k < n; k++) {
        const rtgr_object& o = objs[order[k]];
        // (finite in the kernels' scalar type too: `limit` is its largest value — a centre that becomes inf there has no bounding sphere)
        if (!(std::fabs(o.p[1]) <= limit) || !(std::fabs(o.p[2]) <= limit) || !(std::fabs(o.p[3]) <= limit) || !(std::fabs(o.p[8]) <= limit)) return;
        radii[k] = std::fabs(o.p[8]);
    }
    std::vector<double> sorted = radii;
    std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
    const double big = 4.0 * sorted[n / 2];
    std::vector<uint32_t> loose, rest;
    // (… and an inside-out sphere, R < 0: the resolve kernel's bound for a group's members — select_objects — wants R >= 0)
    for (size_t k = 0; k < n; k++) ((radii[k] > big || objs[order[k]].p[8] < 0) ? loose : rest).push_back(order[k]);
    if (rest.size() < 2 * (size_t)RTGR_GROUP_MAX) return;
    // (leaf = 0: automatic — a few dozen spheres spread over a scene make better groups of <= 4: 2048², 24 objects 35.5 -> 33.8 ms, 32:
    //  42.4 -> 41.4, but 40: 43.9 -> 45.7; profiles/r06/groups_small_lists.log)
    if (leaf == 0) leaf = rest.size() < 36 ? RTGR_GROUP_MAX / 2 : RTGR_GROUP_MAX;
    std::vector<std::pair<size_t, size_t>> todo{{0, rest.size()}}, leaves;
    while (!todo.empty()) {
        const auto [lo, hi] = todo.back();
        todo.pop_back();
        if (hi - lo <= leaf) { leaves.push_back({lo, hi}); continue; }
        double mn[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, mx[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
        for (size_t k = lo; k < hi; k++)
            for (int q = 0; q < 3; q++) { mn[q] = std::min(mn[q], objs[rest[k]].p[1 + q]); mx[q] = std::max(mx[q], objs[rest[k]].p[1 + q]); }
        int ax = 0;
        for (int q = 1; q < 3; q++) if (mx[q] - mn[q] > mx[ax] - mn[ax]) ax = q;
        const size_t mid = lo + (hi - lo) / 2;
        std::nth_element(rest.begin() + lo, rest.begin() + mid, rest.begin() + hi, [&](uint32_t a, uint32_t b) {
            const double ca = objs[a].p[1 + ax], cb = objs[b].p[1 + ax];
            return ca < cb || (ca == cb && a < b);
        });
        todo.push_back({mid, hi});
        todo.push_back({lo, mid});
    }
    std::sort(leaves.begin(), leaves.end());
    for (auto& lf : leaves) std::sort(rest.begin() + lf.first, rest.begin() + lf.second);   // (members in the caller's order)
    *nloose = (uint32_t)loose.size();
    order = loose;
    order.insert(order.end(), rest.begin(), rest.end());
    for (auto& lf : leaves) groups.push_back({(uint32_t)(loose.size() + lf.first), (uint32_t)(lf.second - lf.first)});
    if (leaves.size() < RTGR_SUPER_FROM) return;
    // the second level: the same tree (the splits above cut every range at lo + (hi - lo) / 2), stopped at nodes of <= 8 leaves' worth —
    // more for very long lists: with G groups in runs of r, a step asks G / r runs + r groups of every run it cannot rule out (a few),
    // least for r ~ sqrt(G / 3) (8 up to ~1500 spheres; 70 for 120000)
    const size_t per_run = std::max<size_t>(8, (size_t)std::sqrt((double)leaves.size() / 3.0));
    std::vector<std::pair<size_t, size_t>> nodes;
    todo.assign(1, {0, rest.size()});
    while (!todo.empty()) {
        const auto [lo, hi] = todo.back();
        todo.pop_back();
        if (hi - lo <= per_run * leaf) { nodes.push_back({lo, hi}); continue; }
        const size_t mid = lo + (hi - lo) / 2;
        todo.push_back({mid, hi});
        todo.push_back({lo, mid});
    }
    std::sort(nodes.begin(), nodes.end());
    size_t g = 0;
    for (auto& nd : nodes) {   // (leaves are sorted by position and nest in the nodes)
        const size_t g0 = g;
        while (g < leaves.size() && leaves[g].first < nd.second) g++;
        supers.push_back({(uint32_t)g0, (uint32_t)(g - g0)});
    }
}
// … and a group's bounding sphere from its members AS THE KERNELS SEE THEM (the scalar type's values): centre = the middle of the
// centres' box, radius = max (|c_i − C| + |r_i|), evaluated in double and rounded UP into R with a margin of 64 ulp — what the reach
// test's argument needs is containment, not tightness.
template <class R>
static void bounding_sphere(const DevObject<R>* t, const SphereGroup& g, DevObject<R>& out) {
    double mn[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, mx[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (uint32_t k = g.first; k < g.first + g.count; k++)
        for (int q = 0; q < 3; q++) { mn[q] = std::min(mn[q], (double)t[k].p[1 + q]); mx[q] = std::max(mx[q], (double)t[k].p[1 + q]); }
    std::memset(&out, 0, sizeof out);
    out.kind = RTGR_SPHERE;
    out.type = g.first;
    out.orig = g.count;
    for (int q = 0; q < 3; q++) out.p[1 + q] = (R)(0.5 * mn[q] + 0.5 * mx[q]);
    double rad = 0;
    for (uint32_t k = g.first; k < g.first + g.count; k++) {
        double d2 = 0;
        for (int q = 0; q < 3; q++) { const double e = (double)t[k].p[1 + q] - (double)out.p[1 + q]; d2 += e * e; }
        rad = std::max(rad, std::sqrt(d2) + std::fabs((double)t[k].p[8]));
    }
    rad = rad * (1.0 + 64.0 * (double)std::numeric_limits<R>::epsilon()) + (double)std::numeric_limits<R>::min();
    R r = (R)rad;
    if ((double)r < rad) r = std::nextafter(r, std::numeric_limits<R>::infinity());
    out.p[8] = r;
    object_constants<R>(out);
}
// … and a run of groups' bounding sphere: over ALL the members of its groups (they are neighbours in the device list too)
template <class R>
static void super_sphere(const DevObject<R>* t, const std::vector<SphereGroup>& groups, const SphereGroup& run, DevObject<R>& out) {
    const SphereGroup& a = groups[run.first];
    const SphereGroup& b = groups[run.first + run.count - 1];
    bounding_sphere<R>(t, SphereGroup{a.first, b.first + b.count - a.first}, out);
    out.type = run.first;
    out.orig = run.count;
}

template <class R>
int convert_scene(DeviceCtx& D, const rtgr_scene* s, DevScene<R>& d, const UserModule** user, hipStream_t st) {
    if (!s) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if ((s->metric & ~RTGR_METRIC_GENERIC) > RTGR_GRID) return fail(RTGR_ERR_BAD_ARG, "unknown metric enum");
    *user = nullptr;
    if (s->nobj > RTGR_MAX_OBJECTS && !s->objects)
        return fail(RTGR_ERR_BAD_ARG, "more than RTGR_MAX_OBJECTS objects: hand the list over through rtgr_scene.objects (any length)");
    if (s->nobj > RTGR_OBJECTS_LIMIT) return fail(RTGR_ERR_BAD_ARG, "more than RTGR_OBJECTS_LIMIT objects");
    const rtgr_object* objs = scene_objects(s);
    const bool user_metric = (s->metric & ~RTGR_METRIC_GENERIC) == RTGR_USER;
    const GridTable* grid = nullptr;
    if ((s->metric & ~RTGR_METRIC_GENERIC) == RTGR_GRID) {   // a metric sampled on a grid: rtgr_scene.user_metric is the grid's id
        for (uint32_t o = 0; o < s->nobj; o++)
            if (objs[o].kind == RTGR_USER_OBJECT)
                return fail(RTGR_ERR_BAD_ARG, "RTGR_GRID: user objects (RTGR_USER_OBJECT) in a scene with a grid metric are not supported");
        grid = D.grids.find(s->user_metric);
        if (!grid)
            return fail(RTGR_ERR_BAD_ARG, "RTGR_GRID: no grid metric with id " + std::to_string(s->user_metric) +
                                          " is loaded in this context (rtgr_grid_metric_load; an unloaded id stays unknown)");
    }
    bool user_objects = tl_probe_forces_unit && s->user_metric != 0 && !user_metric;
    for (uint32_t o = 0; o < s->nobj; o++) user_objects = user_objects || objs[o].kind == RTGR_USER_OBJECT;
    if (grid) user_objects = false;   // (rtgr_scene.user_metric names the grid, never a unit)
    if (user_metric || user_objects) {
        const char* what = user_metric ? "RTGR_USER" : "RTGR_USER_OBJECT";
        if (D.modules.empty())
            return fail(RTGR_ERR_BAD_ARG, std::string(what) + ": no run-time unit loaded (rtgr_user_metric_load / rtgr_user_unit_compile)");
        *user = D.find_module(s->user_metric);
        if (!*user)
            return fail(RTGR_ERR_BAD_ARG, std::string(what) + ": rtgr_scene.user_metric names a unit that is not loaded in this "
                                          "context (a scene only ever runs with the kernels of its own unit)");
        const UserModule& U = **user;
        if (user_metric && !U.has_metric)
            return fail(RTGR_ERR_BAD_ARG, "RTGR_USER: this unit defines no metric (it was built for a built-in one: rtgr_user_unit_info)");
        if (user_objects && !U.has_objects)
            return fail(RTGR_ERR_BAD_ARG, "RTGR_USER_OBJECT: this unit's source defines no rtgr_user_distance / rtgr_user_objcolor");
        if (!user_metric) {   // the unit's kernels are ONE built-in metric variant's: the scene's must be that one
            uint32_t mv; bool sp;
            scene_variant(s, &mv, &sp);
            if (U.has_metric || U.metric != mv || U.spin != sp)
                return fail(RTGR_ERR_BAD_ARG, "RTGR_USER_OBJECT: this unit's kernels were built for another metric variant (metric enum / "
                                              "RTGR_METRIC_GENERIC / a != 0 differ from the scene's): build one for THIS scene — "
                                              "rtgr_user_unit_compile(ctx, source, stationary, &scene, &id)");
        }
        if (sizeof(R) != 8 && !U.full10_f32)
            return fail(RTGR_ERR_BAD_ARG, "this unit carries no Float32 kernels");
    }
    std::memset(&d, 0, sizeof d);
    d.metric = s->metric & ~RTGR_METRIC_GENERIC;
    d.nobj = s->nobj;
    d.M = (R)s->M;
    d.a = (R)s->a;
    if (grid) {
        if (grid->axes.dims == 4) d.metric = RTGR_GRID4;   // a time-dependent grid: its own kernels and hooks
        d.grid = dev_grid<R>(*grid);
    }
    int rc;
    const uint32_t n0 = s->nobj < (uint32_t)RTGR_MAX_OBJECTS ? s->nobj : (uint32_t)RTGR_MAX_OBJECTS;
    // the device list is REGROUPED (DevScene, rtgr_args.hpp): spheres first, then the rest, both in the caller's order, every object
    // with its original index — the integrate kernels walk the spheres without a dispatch on the kind; the colour rule breaks ties
    // by the original index and reports it, so no result depends on the regrouping
    std::vector<uint32_t> order;
    order.reserve(s->nobj);
    for (uint32_t o = 0; o < s->nobj; o++) if (objs[o].kind == RTGR_SPHERE) order.push_back(o);
    d.nsph = (uint32_t)order.size();
    // … and the spheres of a LONG list in groups of neighbours (DevScene: GROUPS)
    std::vector<SphereGroup> groups, supers;
    const long kg = tl_knobs_override ? tl_knobs_override->groups : D.knobs.groups;   // (0: off; 1: on; >= 2: on, with that many spheres per group at most — experiments)
    if (s->nobj > n0 && kg)
        group_spheres(objs, order, &d.nloose, groups, supers, kg >= 2 ? (size_t)kg : (size_t)0, (double)std::numeric_limits<R>::max());
    for (uint32_t o = 0; o < s->nobj; o++) if (objs[o].kind != RTGR_SPHERE) order.push_back(o);
    for (uint32_t k = 0; k < n0; k++) {
        if ((rc = convert_object<R>(objs[order[k]], d.obj[k]))) return rc;
        d.obj[k].orig = order[k];
    }
    if (s->nobj > n0) {   // a long list: a device table of ALL of it (+ its groups), shared by every call with the same list
        std::vector<char> content((size_t)(s->nobj + groups.size() + supers.size()) * sizeof(DevObject<R>), 0);
        DevObject<R>* t = (DevObject<R>*)content.data();
        for (uint32_t k = 0; k < s->nobj; k++) {
            if ((rc = convert_object<R>(objs[order[k]], t[k]))) return rc;
            t[k].orig = order[k];
        }
        for (size_t g = 0; g < groups.size(); g++) bounding_sphere<R>(t, groups[g], t[s->nobj + g]);
        for (size_t u = 0; u < supers.size(); u++) super_sphere<R>(t, groups, supers[u], t[s->nobj + groups.size() + u]);
        d.ngroups = (uint32_t)groups.size();
        d.nsuper = (uint32_t)supers.size();
        const void* dev = nullptr;
        if ((rc = object_table(D, content, st, &dev))) return rc;
        d.more = (const DevObject<R>*)dev + n0;
    }
    return RTGR_OK;
}
template <class R>
int convert_solver(const rtgr_solver* s, DevSolver<R>& d) {
    if (!s) return fail(RTGR_ERR_BAD_ARG, "solver is NULL");
    if (!(s->reltol > 0) || !(s->abstol > 0)) return fail(RTGR_ERR_BAD_ARG, "tolerances must be positive");
    if (!(s->lambda1 > s->lambda0)) return fail(RTGR_ERR_BAD_ARG, "lambda1 must exceed lambda0");
    if (s->max_steps == 0) return fail(RTGR_ERR_BAD_ARG, "max_steps must be positive");
    d.reltol = (R)s->reltol;
    d.abstol = (R)s->abstol;
    d.lambda0 = (R)s->lambda0;
    d.lambda1 = (R)s->lambda1;
    d.hit_threshold = (R)s->hit_threshold;
    for (int c = 0; c < 3; c++) d.miss_rgb[c] = (R)s->miss_rgb[c];
    d.max_steps = s->max_steps;
    d.interp_points = s->interp_points;
    return RTGR_OK;
}
template <class R>
void convert_camera(const rtgr_camera* c, DevCamera<R>& d) {
    for (int a = 0; a < 4; a++) {
        d.pos[a] = (R)c->pos[a];
        d.widthx[a] = (R)c->widthx[a];
        d.widthy[a] = (R)c->widthy[a];
        d.normal[a] = (R)c->normal[a];
    }
}
template int convert_scene<double>(DeviceCtx&, const rtgr_scene*, DevScene<double>&, const UserModule**, hipStream_t);
template int convert_scene<float>(DeviceCtx&, const rtgr_scene*, DevScene<float>&, const UserModule**, hipStream_t);
template int convert_solver<double>(const rtgr_solver*, DevSolver<double>&);
template int convert_solver<float>(const rtgr_solver*, DevSolver<float>&);
template void convert_camera<double>(const rtgr_camera*, DevCamera<double>&);
template void convert_camera<float>(const rtgr_camera*, DevCamera<float>&);

}  // namespace rtgr

// A test hook, not part of include/rtgr.h (tests/test_reach_floor.py; host code only — runs without a GPU): the reach test's constants as
// the kernels of the scalar type get them.  Per object, through convert_object: rows[2k] = DevObject::nR2, rows[2k + 1] = ::floor_ (a
// bounding sphere is a sphere of the scalar type's centre and radius: the same function); consts[0..2] = reach_eps, reach_guard,
// reach_guard2 of that type.  Returns 0, or the error of a bad object.
extern "C" int rtgr_testhook_reach_constants(const rtgr_object* objs, uint32_t n, int is_f32, double* rows, double* consts) {
    using namespace rtgr;
    auto fill = [&](auto zero) -> int {
        typedef decltype(zero) R;
        consts[0] = (double)reach_eps<R>(); consts[1] = (double)reach_guard<R>(); consts[2] = (double)reach_guard2<R>();
        for (uint32_t k = 0; k < n; k++) {
            DevObject<R> d;
            if (int rc = convert_object<R>(objs[k], d)) return rc;
            rows[2 * k] = (double)d.nR2;
            rows[2 * k + 1] = (double)d.floor_;
        }
        return RTGR_OK;
    };
    return is_f32 ? fill(0.0f) : fill(0.0);
}

// A test hook, not part of include/rtgr.h (tests/test_host_logic.py; host code only — runs without a GPU): how convert_scene lays a
// list's SPHERES out — `order` (n entries: indices into objs, loose spheres first, then the groups' members), the number of loose
// ones, and per group {centre x, y, z, radius, first position, count} as the kernels of the scalar type get them.  objs[] must all be
// RTGR_SPHEREs.  Returns the number of groups (0: the list gets none), or -1 when `cap` rows do not hold them; *nsuper rows of runs of
// groups follow the groups' rows (first / count: group indices).
extern "C" int rtgr_testhook_group_spheres(const rtgr_object* objs, uint32_t n, int is_f32, uint32_t* order_out, uint32_t* nloose,
                                           double* groups_out, uint32_t cap, uint32_t* nsuper) {
    using namespace rtgr;
    std::vector<uint32_t> order(n);
    for (uint32_t k = 0; k < n; k++) order[k] = k;
    std::vector<SphereGroup> groups, supers;
    group_spheres(objs, order, nloose, groups, supers, 0, is_f32 ? (double)std::numeric_limits<float>::max() : std::numeric_limits<double>::max());
    for (uint32_t k = 0; k < n; k++) order_out[k] = order[k];
    if (groups.size() + supers.size() > cap) return -1;
    if (nsuper) *nsuper = (uint32_t)supers.size();
    auto fill = [&](auto zero) {
        typedef decltype(zero) R;
        std::vector<DevObject<R>> t(n);
        for (uint32_t k = 0; k < n; k++) (void)convert_object<R>(objs[order[k]], t[k]);
        for (size_t g = 0; g < groups.size(); g++) {
            DevObject<R> G;
            bounding_sphere<R>(t.data(), groups[g], G);
            double* o = groups_out + 6 * g;
            o[0] = (double)G.p[1]; o[1] = (double)G.p[2]; o[2] = (double)G.p[3]; o[3] = (double)G.p[8]; o[4] = G.type; o[5] = G.orig;
        }
        for (size_t u = 0; u < supers.size(); u++) {   // (the runs of groups follow the groups; first / count are group indices)
            DevObject<R> G;
            super_sphere<R>(t.data(), groups, supers[u], G);
            double* o = groups_out + 6 * (groups.size() + u);
            o[0] = (double)G.p[1]; o[1] = (double)G.p[2]; o[2] = (double)G.p[3]; o[3] = (double)G.p[8]; o[4] = G.type; o[5] = G.orig;
        }
    };
    if (is_f32) fill(0.0f); else fill(0.0);
    return (int)groups.size();
}
