// rtgr_objects.hpp — everything about `Object` (src/RayTraceGR.jl:374-441, :513-533): the ONE place a new object kind is taught.
#pragma once
#include "rtgr_physics.hpp"

namespace rtgr {

// ---- objects (src/RayTraceGR.jl:374-441) -------------------------------------------------------------------------------
// `Object{T}` is an open abstract type with two methods, distance and objcolor (:374-389).  A run-time unit whose source
// defines them (rtgr_user_unit.hip.in sets RTGR_USER_OBJECTS) supplies
//     template <class S> __device__ S    rtgr_user_distance(unsigned type, const S x[4], const S p[9]);
//     template <class S> __device__ void rtgr_user_objcolor(unsigned type, const S x[4], const S p[9], S rgb[3]);
// and, optionally (RTGR_USER_REACH), the bound the FAR pass needs to skip a step's scan:
//     template <class S> __device__ S    rtgr_user_reach(unsigned type, const S x[4], const S p[9], const S dl[4]);
//     >= |distance(x') − distance(x)| for every x' with |x'_q − x_q| <= dl[q]
// (include/rtgr.h "user objects").  The library's own kernels are compiled without them: a scene with an RTGR_USER_OBJECT
// only ever runs with the kernels of its unit (convert_scene, rtgr_scene_host.hip).
#ifdef RTGR_USER_OBJECTS
template <class S> __device__ S rtgr_user_distance(unsigned type, const S x[4], const S p[9]);
template <class S> __device__ void rtgr_user_objcolor(unsigned type, const S x[4], const S p[9], S rgb[3]);
#ifdef RTGR_USER_REACH
template <class S> __device__ S rtgr_user_reach(unsigned type, const S x[4], const S p[9], const S dl[4]);
#endif
#ifdef RTGR_USER_SAMPLE
template <class S> __device__ bool rtgr_user_sample(unsigned type, S p[9]);   // optional: a sample object of `type` for the load-time probe
#endif
#endif

template <class R>
RTGR_DEV R obj_distance(const DevObject<R>& o, const R pos[4]) {
    if (o.kind == RTGR_PLANE) return pos[0] - o.p[0];                                    // :399-401
    if (o.kind == RTGR_SPHERE) {                                                         // :415-419
        const R dx = pos[1] - o.p[1], dy = pos[2] - o.p[2], dz = pos[3] - o.p[3];
        const R Rr = o.p[8];
        const R d = rfma(dx, dx, rfma(dy, dy, rfma(dz, dz, -Rr * Rr)));
        return Rr < R(0) ? -d : d;  // sign(R)*( … ); R = 0 never used
    }
#ifdef RTGR_USER_OBJECTS
    if (o.kind == RTGR_USER_OBJECT) return rtgr_user_distance<R>(o.type, pos, o.p);     // distance(obj::MyThing, pos)  :377-386
#endif
    // RTGR_DISK: max(|z|−h, r_in−ϱ, ϱ−r_out)
    const R rc = rsqrt_(rfma(pos[1], pos[1], pos[2] * pos[2]));
    R d = rabs(pos[3]) - o.p[0];
    d = rmax(d, o.p[1] - rc);
    d = rmax(d, rc - o.p[2]);
    return d;
}

// The disk's distance as the ContinuousCallback SCAN needs it: its sign only (the scan multiplies the minimum over the
// objects by the sign at the step start and tests < 0 / <= 0; the minimum's sign is fixed by its members' signs).  The two
// radial terms r_in − ϱ and ϱ − r_out are replaced by THEIR SIGNS, read off s = x² + y² without taking the root: the host
// precomputes, in the device's scalar type, the band of s whose correctly rounded square root equals the radius
// (p[3] = min{s : √s >= r_in}, p[4] = min{s : √s > r_in}, p[5], p[6] likewise for r_out; disk_sqrt_band, rtgr_scene_host.hip), so
//     sign(r_in − RN(√s)) = +1 for s < p[3], 0 for p[3] <= s < p[4], −1 otherwise
// EXACTLY — same sign, zero included, as obj_distance computes with its IEEE square root, for every s (√ is monotone and
// correctly rounded).  Nine IEEE roots (~16 instructions each) per accepted NEAR step become compares and selects; the true
// distance is still what the event root-finder (resolve_kernel) and the colouring see.
template <class R>
RTGR_DEV R disk_sign_distance(const DevObject<R>& o, R px, R py, R pz) {
    const R s = rfma(px, px, py * py);
    const R e_in = s < o.p[3] ? R(1) : (s < o.p[4] ? R(0) : R(-1));     // sign(r_in − ϱ)
    const R e_out = s < o.p[5] ? R(-1) : (s < o.p[6] ? R(0) : R(1));    // sign(ϱ − r_out)
    return rmax(rmax(rabs(pz) - o.p[0], e_in), e_out);
}

// … and as the FAR pass's reach bound needs it: its magnitude, to ~1e-16 relative (the bound carries a 1e-6 guard), from
// the 6-instruction reciprocal square root instead of the IEEE expansion.
template <class R>
RTGR_DEV R disk_distance_fast(const DevObject<R>& o, R px, R py, R pz) {
    const R s = rfma(px, px, py * py);
    const R rc = s > R(0) ? s * frsq<R>(s) : R(0);
    return rmax(rmax(rabs(pz) - o.p[0], o.p[1] - rc), rc - o.p[2]);
}

// The object list in order — f(object, index) —, as `for obj in objs` walks the reference's Vector (:434, :520): the first
// RTGR_MAX_OBJECTS objects from the kernels' argument block (a wave-uniform index into the kernarg segment: scalar loads), the
// rest of a longer list from the scene's device table (DevScene::more; the same wave-uniform walk over global memory).  The second
// loop is cold code for every scene of up to RTGR_MAX_OBJECTS objects: never entered, and outside the hot loop's instruction
// stream.
template <class R, class F>
RTGR_DEV void for_each_object(const DevScene<R>& sc, F&& f) {
    const uint32_t n0 = sc.nobj < (uint32_t)RTGR_MAX_OBJECTS ? sc.nobj : (uint32_t)RTGR_MAX_OBJECTS;
    for (uint32_t o = 0; o < n0; o++) f(sc.obj[o], o);
#ifndef RTGR_INLINE_OBJECTS_ONLY   // (A/B builds: the loop as it was before lists could be longer — tools/launch_ab.py builds)
    if (__builtin_expect(sc.nobj > (uint32_t)RTGR_MAX_OBJECTS, 0)) {   // (laid out of line: 0.4-0.7 % of the 4096² frame when it sat in the hot loop's stream)
        // The table is read-only for the kernel's lifetime and walked with a wave-uniform index: through the CONSTANT address space
        // its loads are scalar loads (s_load, the scalar cache — what the kernarg-resident objects get), not vector loads of one
        // address by 64 lanes with a vector-memory round trip ahead of every object's arithmetic (measured at 64 objects, 2048²:
        // the table walked with global_load cost the frame 3 x what its instruction count explains — DESIGN.md §4.7).
        typedef const DevObject<R> __attribute__((address_space(4))) * ConstTable;
        const ConstTable more = (ConstTable)(unsigned long long)sc.more;
        for (uint32_t o = (uint32_t)RTGR_MAX_OBJECTS; o < sc.nobj; o++)
            f(*(const DevObject<R>*)(more + (o - (uint32_t)RTGR_MAX_OBJECTS)), o);
    }
#endif
}
// The same walk with the spheres — objects [0, nsph) of the regrouped list (DevScene) — handed to a function of their own:
// fs(sphere, position) needs no dispatch on the kind, fo(object, position) is the general one.  For consumers that do not care
// about the order (the reach test's conjunction, the minima of the sample-point scan).
template <class R, class FS, class FO>
RTGR_DEV void for_each_by_kind(const DevScene<R>& sc, FS&& fs, FO&& fo) {
    const uint32_t n0 = sc.nobj < (uint32_t)RTGR_MAX_OBJECTS ? sc.nobj : (uint32_t)RTGR_MAX_OBJECTS;
    const uint32_t s0 = sc.nsph < n0 ? sc.nsph : n0;
    for (uint32_t o = 0; o < s0; o++) fs(sc.obj[o], o);
    for (uint32_t o = s0; o < n0; o++) fo(sc.obj[o], o);
#ifndef RTGR_INLINE_OBJECTS_ONLY
    if (__builtin_expect(sc.nobj > (uint32_t)RTGR_MAX_OBJECTS, 0)) {
        typedef const DevObject<R> __attribute__((address_space(4))) * ConstTable;
        const ConstTable more = (ConstTable)(unsigned long long)sc.more;
        const uint32_t s1 = sc.nsph < sc.nobj ? sc.nsph : sc.nobj;
        for (uint32_t o = (uint32_t)RTGR_MAX_OBJECTS; o < s1; o++) fs(*(const DevObject<R>*)(more + (o - (uint32_t)RTGR_MAX_OBJECTS)), o);
        for (uint32_t o = s1 > (uint32_t)RTGR_MAX_OBJECTS ? s1 : (uint32_t)RTGR_MAX_OBJECTS; o < sc.nobj; o++)
            fo(*(const DevObject<R>*)(more + (o - (uint32_t)RTGR_MAX_OBJECTS)), o);
    }
#endif
}
// The sample-point scan's walk (integrate_body): the objects whose bit — bit (position >> shift) — is set in `mask`, spheres to fs,
// the other kinds to fo.  A list in the argument block is walked object by object with the bit tested on the way (the hot loop's
// stream); a longer one BY THE SET BITS, through the device table: the scan of a step that can meet three of 100000 objects is not
// a walk over 100000 bits.
template <class R, class FS, class FO>
RTGR_DEV void for_each_masked_by_kind(const DevScene<R>& sc, unsigned long long mask, uint32_t shift, FS&& fs, FO&& fo) {
#ifndef RTGR_INLINE_OBJECTS_ONLY
    if (__builtin_expect(sc.nobj > (uint32_t)RTGR_MAX_OBJECTS, 0)) {
        typedef const DevObject<R> __attribute__((address_space(4))) * ConstTable;
        const ConstTable table = (ConstTable)(unsigned long long)(sc.more - (uint32_t)RTGR_MAX_OBJECTS);
        unsigned long long m = mask;
        while (m != 0ull) {
            const uint32_t b = (uint32_t)__builtin_ctzll(m);
            m &= m - 1ull;
            const uint32_t o0 = b << shift;
            uint32_t o1 = o0 + (1u << shift);
            o1 = o1 < sc.nobj ? o1 : sc.nobj;
            for (uint32_t o = o0; o < o1; o++) {
                if (o < sc.nsph) fs(*(const DevObject<R>*)(table + o), o);
                else fo(*(const DevObject<R>*)(table + o), o);
            }
        }
        return;
    }
#endif
    const uint32_t n0 = sc.nobj < (uint32_t)RTGR_MAX_OBJECTS ? sc.nobj : (uint32_t)RTGR_MAX_OBJECTS;   // (such a list has one bit per object: shift = 0)
    const uint32_t s0 = sc.nsph < n0 ? sc.nsph : n0;
    for (uint32_t o = 0; o < s0; o++) if ((mask >> o) & 1ull) fs(sc.obj[o], o);
    for (uint32_t o = s0; o < n0; o++) if ((mask >> o) & 1ull) fo(sc.obj[o], o);
}
// The reach test's walk (integrate_body, select_objects): as for_each_by_kind, but a list with GROUPS (DevScene, rtgr_args.hpp) is walked group
// by group — fg(group, level) -> wave-uniform "some lane cannot rule this group out"; only then its members are handed to fs.  With a
// second level (nsuper > 0) the runs of groups are asked first (level 1), their groups (level 0) only when a run is not ruled out.  The
// whole walk of a grouped list reads the device table (scalar loads through the constant address space, as above) and is cold code for
// every list without groups.
template <class R, class FG, class FS, class FO>
RTGR_DEV void for_each_within_reach(const DevScene<R>& sc, FG&& fg, FS&& fs, FO&& fo) {
#ifndef RTGR_INLINE_OBJECTS_ONLY
    if (__builtin_expect(sc.ngroups != 0u, 0)) {
        typedef const DevObject<R> __attribute__((address_space(4))) * ConstTable;
        const ConstTable table = (ConstTable)(unsigned long long)(sc.more - (uint32_t)RTGR_MAX_OBJECTS);
        const ConstTable groups = table + sc.nobj;
        const ConstTable supers = groups + sc.ngroups;
        for (uint32_t o = 0; o < sc.nloose; o++) fs(*(const DevObject<R>*)(table + o), o);
        const uint32_t runs = sc.nsuper != 0u ? sc.nsuper : 1u;
        for (uint32_t s = 0; s < runs; s++) {
            uint32_t g0 = 0u, g1 = sc.ngroups;
            if (sc.nsuper != 0u) {
                const DevObject<R>& S = *(const DevObject<R>*)(supers + s);
                if (!fg(S, 1)) continue;
                g0 = S.type;
                g1 = S.type + S.orig;
            }
            for (uint32_t g = g0; g < g1; g++) {
                const DevObject<R>& G = *(const DevObject<R>*)(groups + g);
                if (fg(G, 0)) {
                    const uint32_t o1 = G.type + G.orig;
                    for (uint32_t o = G.type; o < o1; o++) fs(*(const DevObject<R>*)(table + o), o);
                }
            }
        }
        for (uint32_t o = sc.nsph; o < sc.nobj; o++) fo(*(const DevObject<R>*)(table + o), o);
        return;
    }
#endif
    for_each_by_kind<R>(sc, fs, fo);
}
// A SAMPLE of a grouped list (ngroups > 0): the loose spheres, ONE member of every group (of every run of groups, where there are
// runs), the other kinds — f(object, position).
template <class R, class F>
RTGR_DEV void for_each_sample(const DevScene<R>& sc, F&& f) {
    typedef const DevObject<R> __attribute__((address_space(4))) * ConstTable;
    const ConstTable table = (ConstTable)(unsigned long long)(sc.more - (uint32_t)RTGR_MAX_OBJECTS);
    const ConstTable groups = table + sc.nobj;
    for (uint32_t o = 0; o < sc.nloose; o++) f(*(const DevObject<R>*)(table + o), o);
    if (sc.nsuper != 0u) {   // (with a second level: one member of every RUN of groups — the bound only has to be a bound)
        const ConstTable supers = groups + sc.ngroups;
        for (uint32_t s = 0; s < sc.nsuper; s++) {
            const uint32_t g = ((const DevObject<R>*)(supers + s))->type;
            const uint32_t o = ((const DevObject<R>*)(groups + g))->type;
            f(*(const DevObject<R>*)(table + o), o);
        }
    } else {
        for (uint32_t g = 0; g < sc.ngroups; g++) {
            const uint32_t o = ((const DevObject<R>*)(groups + g))->type;
            f(*(const DevObject<R>*)(table + o), o);
        }
    }
    for (uint32_t o = sc.nsph; o < sc.nobj; o++) f(*(const DevObject<R>*)(table + o), o);
}
// … and one object by (per-lane) POSITION in the regrouped list
template <class R>
RTGR_DEV const DevObject<R>& object_at(const DevScene<R>& sc, uint32_t o) {
    return o < (uint32_t)RTGR_MAX_OBJECTS ? sc.obj[o] : sc.more[o - (uint32_t)RTGR_MAX_OBJECTS];
}

// A SELECTION of the list's objects (the resolve kernel, rtgr_resolve.hpp: select_objects): bit o >> shift of the mask says
// whether object o (position in the device list) takes part.  Only ever used to leave out objects that provably cannot be the minimum.
struct ObjSel {
    unsigned long long mask;
    uint32_t shift;
    // lists beyond 64 objects (a bit is 2, 4, … 2048 neighbours): the selected positions themselves, entry k in lane k of `list`
    // (read with v_readlane, which ignores EXEC), `count` of them; count > 64: too many, walk the mask's blocks
    uint32_t list;
    uint32_t count;
    RTGR_DEV bool has(uint32_t o) const { return ((mask >> (o >> shift)) & 1ull) != 0ull; }
    RTGR_DEV void add(uint32_t o) {   // wave-uniform o
        mask |= 1ull << (o >> shift);
        if (shift != 0u) {
            if (count < 64u) list = ((threadIdx.x & 63u) == count) ? o : list;   // (called with every lane of the wave active: select_objects)
            count++;
        }
    }
};
RTGR_DEV uint32_t objsel_shift(uint32_t nobj) {   // the smallest shift with (nobj − 1) >> shift <= 63
    return nobj > 64u ? 32u - (uint32_t)__builtin_clz((nobj - 1u) >> 6) : 0u;
}

// The objects of a selection, in list order — f(object, position) —, found by the mask's set bits (a list of 1024 objects is not walked
// to find the three that are selected).  Lists beyond the argument block only: the device table holds the whole list.
template <class R, class F>
RTGR_DEV void for_each_selected(const DevScene<R>& sc, ObjSel sel, F&& f) {
    typedef const DevObject<R> __attribute__((address_space(4))) * ConstTable;
    const ConstTable table = (ConstTable)(unsigned long long)(sc.more - (uint32_t)RTGR_MAX_OBJECTS);
    if (sel.shift != 0u && sel.count <= 64u) {   // by the list of positions
        for (uint32_t k = 0; k < sel.count; k++) {
            const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)sel.list, (int)k);
            f(*(const DevObject<R>*)(table + o), o);
        }
        return;
    }
    unsigned long long m = sel.mask;
    while (m != 0ull) {
        const uint32_t b = (uint32_t)__builtin_ctzll(m);
        m &= m - 1ull;
        const uint32_t o0 = b << sel.shift;
        uint32_t o1 = o0 + (1u << sel.shift);
        o1 = o1 < sc.nobj ? o1 : sc.nobj;
        for (uint32_t o = o0; o < o1; o++) f(*(const DevObject<R>*)(table + o), o);
    }
}

template <class R, bool SEL = false>
RTGR_DEV R min_distance(const DevScene<R>& sc, const R pos[4], ObjSel sel = ObjSel{}) {   // :433-441
    R dmin = R(__builtin_huge_val());
    auto fold = [&](const DevObject<R>& ob, uint32_t) {
        const R d = obj_distance<R>(ob, pos);
        dmin = (d < dmin || d != d) ? d : dmin;
    };
    if constexpr (SEL) for_each_selected<R>(sc, sel, fold);
    else for_each_object<R>(sc, fold);
    return dmin;
}

// ---- a step against the objects: its position polynomial x(θ) = x + θ c1 + θ² c2 + θ³ c3 + θ⁴ c4 (REC_C), the scan's folds, the reach bounds
// (the packed Float32 pass, rtgr_packed_f32.hpp, shares the sphere forms; its plane and disk forms — two rays per lane — are twins there)
template <class R>
RTGR_DEV void poly_pos(const R x[4], const R cc[4][4], R th, R out[4]) {
#pragma unroll
    for (int q = 0; q < 4; q++) out[q] = rfma(th, rfma(th, rfma(th, rfma(th, cc[3][q], cc[2][q]), cc[1][q]), cc[0][q]), x[q]);
}

// distances of a SPHERE at P sample positions folded into dmin[] (the leading objects of the regrouped list, DevScene: no dispatch on the
// kind).  V: the positions' type — R, or float2 for the packed Float32 pass, which holds two rays against one float object.
template <class R, int P, class V>
RTGR_DEV void fold_sphere(const DevObject<R>& o, const V (&pos)[P][4], V (&dmin)[P]) {
    const V cx = V(o.p[1]), cy = V(o.p[2]), cz = V(o.p[3]);
    const R Rr = o.p[8];
    const V nR2 = V(o.nR2);   // −R², formed once by the host (object_constants) — the same bits the kernel's own −Rr·Rr gives
    if (Rr < R(0)) {                                                                   // :415-419, sign(R) * (|x − c|² − R²)
#pragma unroll
        for (int p = 0; p < P; p++) {
            const V dx = pos[p][1] - cx, dy = pos[p][2] - cy, dz = pos[p][3] - cz;
            dmin[p] = rmin<V>(dmin[p], -rfma<V>(dx, dx, rfma<V>(dy, dy, rfma<V>(dz, dz, nR2))));
        }
    } else {
#pragma unroll
        for (int p = 0; p < P; p++) {
            const V dx = pos[p][1] - cx, dy = pos[p][2] - cy, dz = pos[p][3] - cz;
            dmin[p] = rmin<V>(dmin[p], rfma<V>(dx, dx, rfma<V>(dy, dy, rfma<V>(dz, dz, nR2))));
        }
    }
}

// … of one object of any kind (object-major: parameters fetched once)
template <class R, int P>
RTGR_DEV void fold_distances(const DevObject<R>& o, const R (&pos)[P][4], R (&dmin)[P]) {
    if (o.kind == RTGR_PLANE) {                                                        // src/RayTraceGR.jl:399-401
        const R tm = o.p[0];
#pragma unroll
        for (int p = 0; p < P; p++) dmin[p] = rmin(dmin[p], pos[p][0] - tm);
    } else if (o.kind == RTGR_SPHERE) {                                                // :415-419
        fold_sphere<R, P>(o, pos, dmin);
#ifdef RTGR_USER_OBJECTS
    } else if (o.kind == RTGR_USER_OBJECT) {                                           // the unit's own distance method (:377-386)
#pragma unroll
        for (int p = 0; p < P; p++) dmin[p] = rmin(dmin[p], rtgr_user_distance<R>(o.type, pos[p], o.p));
#endif
    } else {
        // RTGR_DISK: the scan needs the distance's SIGN only — disk_sign_distance reads it off x² + y² without a square
        // root, exactly (above).  The asm barrier pins the operands inside this branch: without it LLVM hoists
        // the (loop-invariant) x² + y² of every sample point out of the object loop, for scenes that contain no disk at all.
#pragma unroll
        for (int p = 0; p < P; p++) {
            R px = pos[p][1], py = pos[p][2];
            asm volatile("" : "+v"(px), "+v"(py));
            dmin[p] = rmin(dmin[p], disk_sign_distance<R>(o, px, py, pos[p][3]));
        }
    }
}

// REACH.  Over a step every coordinate stays in a box |x_q(θ) − x_q| <= dl[q].  A sphere's (or bounding sphere's) distance D0 = |X|² − R²,
// X = x − c, then moves by at most B = Σ_q δ_q (2|X_q| + δ_q).
// (V: as for fold_sphere.  WALK: the object comes from a wave-uniform walk of the list — its −R² is then read from its SGPRs, rfma_sacc)
template <class R, class V, bool WALK = false>
RTGR_DEV void sphere_reach_terms(const DevObject<R>& o, const V x[4], const V dl[4], V& D0, V& B) {
    const V X0 = x[1] - V(o.p[1]), X1 = x[2] - V(o.p[2]), X2 = x[3] - V(o.p[3]);
    V D2;
    if constexpr (WALK) D2 = rfma_sacc<V, R>(X2, X2, o.nR2);
    else D2 = rfma<V>(X2, X2, V(o.nR2));
    D0 = rfma<V>(X0, X0, rfma<V>(X1, X1, D2));
    B = rfma<V>(dl[1], rfma<V>(V(R(2)), rabs<V>(X0), dl[1]),
                rfma<V>(dl[2], rfma<V>(V(R(2)), rabs<V>(X1), dl[2]), dl[3] * rfma<V>(V(R(2)), rabs<V>(X2), dl[3])));
}
// The step cannot change the sign of D0 when |D0| exceeds the move, with its 1e-6 guard, plus a floor of 256 ulp of the operands'
// magnitude |D0| + 2R² (a distance that is itself rounding noise must go through the real scan): out of reach iff lhs > rhs.
//     |D0| > guard B + e (|D0| + 2R²)   <=>   |D0| (1 − e) > guard B + 2 e R²   <=   |D0| − g2 B > F,
// g2 = guard (1 + 2e), F = 2 e R² (1 + 2e) (1 / (1 − e) < 1 + 2e; rtgr_args.hpp: reach_guard2, DevObject::floor_ — formed once, by the
// host).  So lhs = fma(−g2, B, |D0|) against rhs = F: ONE fma and a compare after D0 and B, each with a single scalar operand (an fma of
// g2, B and F would read two, and the second costs a v_mov pair).  Rounding to nearest is monotone and F is a value of R: the rounded
// lhs > F only if the exact |D0| − g2 B > F, and g2 carries a relative slack of e − ulp against its own rounding — the criterion IMPLIES
// the term-by-term one (tests/test_reach_floor.py), the FAR pass hands over every ray it handed over before, and the frame is the same
// bit for bit.  ABS = false: the group form, D0 itself instead of |D0| ("outside the bounding sphere").
// -DRTGR_REACH_TERMWISE_FLOOR=1 builds the term-by-term floor instead (R², 2R², the magnitude and its scaling formed per step and per
// object, with vector arithmetic on wave-uniform data): an experiment flag for timing one against the other.
#ifndef RTGR_REACH_TERMWISE_FLOOR
#define RTGR_REACH_TERMWISE_FLOOR 0
#endif
template <class R, bool ABS, class V>
RTGR_DEV void sphere_reach(const DevObject<R>& o, const V x[4], const V dl[4], V& lhs, V& rhs) {
#if RTGR_REACH_TERMWISE_FLOOR
    const V X0 = x[1] - V(o.p[1]), X1 = x[2] - V(o.p[2]), X2 = x[3] - V(o.p[3]);
    const R Rr = o.p[8];
    const V D0 = rfma<V>(X0, X0, rfma<V>(X1, X1, rfma<V>(X2, X2, V(-Rr * Rr))));
    const V B = rfma<V>(dl[1], rfma<V>(V(R(2)), rabs<V>(X0), dl[1]),
                        rfma<V>(dl[2], rfma<V>(V(R(2)), rabs<V>(X1), dl[2]), dl[3] * rfma<V>(V(R(2)), rabs<V>(X2), dl[3])));
    const V mag = rabs<V>(D0) + V(R(2) * Rr * Rr);
    lhs = ABS ? rabs<V>(D0) : D0;
    rhs = rfma<V>(V(reach_guard<R>()), B, V(reach_eps<R>()) * mag);
#else
    V D0, B;
    sphere_reach_terms<R, V, true>(o, x, dl, D0, B);
    lhs = rfma<V>(V(-reach_guard2<R>()), B, ABS ? rabs<V>(D0) : D0);
    rhs = V(o.floor_);
#endif
}
// … and a plane's distance d = x_t − p0 moves by at most δ_t; floor: 256 ulp of |x_t| + |p0| <= |d| + 2|p0|, folded the same way, Fp = 2 e |p0| (1 + 2e)
template <class R, class V>
RTGR_DEV void plane_reach(const DevObject<R>& o, const V x[4], const V dl[4], V& lhs, V& rhs) {
    const V d = x[0] - V(o.p[0]);
#if RTGR_REACH_TERMWISE_FLOOR
    lhs = rabs<V>(d);
    rhs = rfma<V>(V(reach_guard<R>()), dl[0], V(reach_eps<R>()) * (rabs<V>(x[0]) + V(rabs<R>(o.p[0]))));
#else
    lhs = rfma<V>(V(-reach_guard2<R>()), dl[0], rabs<V>(d));
    rhs = V(o.floor_);
#endif
}
// … and of any object, as an interval: its distance stays within [lower, upper] over the step (guards: select_objects, rtgr_resolve.hpp)
template <class R>
RTGR_DEV void distance_bounds(const DevObject<R>& ob, const R x[4], const R dl[4], R* lower, R* upper) {
    const R eps = sizeof(R) == 8 ? R(2.220446049250313e-16) : R(1.1920929e-7);
    const R guard = R(1) + R(1e-6);
    R d0, B, mag;
    if (ob.kind == RTGR_SPHERE) {   // (the interval keeps its term-by-term floor: it is formed once per event, not once per step)
        R D0;
        sphere_reach_terms<R, R>(ob, x, dl, D0, B);
        mag = rabs(D0) + R(-2) * ob.nR2;
        d0 = ob.p[8] < R(0) ? -D0 : D0;
    } else if (ob.kind == RTGR_PLANE) {
        d0 = x[0] - ob.p[0];
        B = dl[0];
        mag = rabs(x[0]) + rabs(ob.p[0]);
#ifdef RTGR_USER_OBJECTS
    } else if (ob.kind == RTGR_USER_OBJECT) {
#ifdef RTGR_USER_REACH
        const R gd[4] = {guard * dl[0], guard * dl[1], guard * dl[2], guard * dl[3]};
        d0 = rtgr_user_distance<R>(ob.type, x, ob.p);
        B = rtgr_user_reach<R>(ob.type, x, ob.p, gd);
        mag = R(1) + rabs(d0);
#else
        d0 = R(0); B = R(__builtin_huge_val()); mag = R(0);   // no bound given: always in, never bounds the minimum
#endif
#endif
    } else {   // RTGR_DISK: a maximum of three terms moves by at most the largest of their moves
        d0 = obj_distance<R>(ob, x);
        B = rmax(dl[3], dl[1] + dl[2]);
        mag = rabs(d0) + rabs(x[1]) + rabs(x[2]) + rabs(x[3]) + rabs(ob.p[2]);
    }
    const R w = rfma(guard, B, R(256) * eps * mag);
    *lower = d0 - w;
    *upper = d0 + w;
}

// ---- colouring rule of trace_rays (src/RayTraceGR.jl:513-533) + objcolor (:402-404, :420-428) --------------------
template <class R> RTGR_DEV R racos(R x);
template <> RTGR_DEV double racos<double>(double x) { return acos(x); }
template <> RTGR_DEV float racos<float>(float x) { return acosf(x); }
template <class R> RTGR_DEV R ratan2(R y, R x);
template <> RTGR_DEV double ratan2<double>(double y, double x) { return atan2(y, x); }
template <> RTGR_DEV float ratan2<float>(float y, float x) { return atan2f(y, x); }
template <class R> RTGR_DEV R rfloor(R x);
template <> RTGR_DEV double rfloor<double>(double x) { return floor(x); }
template <> RTGR_DEV float rfloor<float>(float x) { return floorf(x); }

template <class R>
RTGR_DEV R mod1(R x) {  // Julia mod(x, 1)
    R r = x - rfloor<R>(x);
    return r >= R(1) ? R(0) : r;
}

template <class R, bool SEL = false>
RTGR_DEV uint32_t colour_pixel(const DevScene<R>& sc, const DevSolver<R>& opt, const R x[4], R col[3], ObjSel sel = ObjSel{}) {
    uint32_t omin = 0, pmin = 0;   // omin: 1-based index in the CALLER's list (what :518-530 calls omin); pmin: position in the device list
    R dmin = opt.hit_threshold;                                                       // :519
    // (the device list is regrouped — spheres first, DevScene —: "the first object with the smallest distance wins" (:520-526) is
    //  the smallest distance and, among equal ones, the smallest ORIGINAL index)
    auto nearest = [&](const DevObject<R>& o_, uint32_t o) {                          // :520-526
        const R d = obj_distance<R>(o_, x);
        if (d < dmin || (d == dmin && omin != 0u && o_.orig + 1u < omin)) { omin = o_.orig + 1u; pmin = o; dmin = d; }
    };
    if constexpr (SEL) for_each_selected<R>(sc, sel, nearest);   // (the rest: provably farther than the nearest object, select_objects)
    else for_each_object<R>(sc, nearest);
    if (omin == 0) {                                                                  // :527-528
        col[0] = opt.miss_rgb[0]; col[1] = opt.miss_rgb[1]; col[2] = opt.miss_rgb[2];
        return 0;
    }
    // (a selection exists for lists beyond the argument block only: their table holds the whole list)
    const DevObject<R>& ob = SEL ? (sc.more - (uint32_t)RTGR_MAX_OBJECTS)[pmin] : object_at<R>(sc, pmin);
    const R pi = R(3.14159265358979323846264338327950288L);
    if (ob.kind == RTGR_PLANE) {                                                      // :402-404
        col[0] = R(0); col[1] = R(0.5); col[2] = R(0);
    } else if (ob.kind == RTGR_SPHERE) {                                              // :420-428
        const R dx = x[1] - ob.p[1], dy = x[2] - ob.p[2], dz = x[3] - ob.p[3];
        const R r = rsqrt_(dx * dx + dy * dy + dz * dz);
        const R th = racos<R>(dz / r);
        const R ph = ratan2<R>(dy, dx);
        col[0] = mod1<R>(R(12) * th / pi);
        col[1] = mod1<R>(R(12) * ph / pi);
        col[2] = R(1);
#ifdef RTGR_USER_OBJECTS
    } else if (ob.kind == RTGR_USER_OBJECT) {                                         // objcolor(obj::MyThing, pos)  :387-389
        rtgr_user_objcolor<R>(ob.type, x, ob.p, col);
#endif
    } else {  // RTGR_DISK — no reference counterpart
        const R rc = rsqrt_(x[1] * x[1] + x[2] * x[2]);
        const R ph = ratan2<R>(x[2], x[1]);
        col[0] = R(1);
        col[1] = mod1<R>(rc);
        col[2] = mod1<R>(R(12) * ph / pi);
    }
    const R scale = R(omin) / R(sc.nobj);                                             // :530
    col[0] *= scale; col[1] *= scale; col[2] *= scale;
    return omin;
}

// parity hook rtgr_eval_objects_f64 / _f32: distance(obj, x) of every object (:377-419), min_distance (:433-441) and the colour rule
// (:513-533) at one point per thread — a body function: a unit with user objects wraps it in a kernel of its own
template <class R>
RTGR_DEV void eval_objects_body(const DevScene<R>& sc, const DevSolver<R>& opt, const R* x, uint64_t n, R* d, R* dmin, uint8_t* hit, R* rgb) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const R xp[4] = {x[4 * p], x[4 * p + 1], x[4 * p + 2], x[4 * p + 3]};
    if (d) for_each_object<R>(sc, [&](const DevObject<R>& ob, uint32_t) { d[p * sc.nobj + ob.orig] = obj_distance<R>(ob, xp); });   // (scene order)
    if (dmin) dmin[p] = min_distance<R>(sc, xp);
    R col[3];
    const uint32_t h = colour_pixel<R>(sc, opt, xp, col);
    if (hit) hit[p] = (uint8_t)h;   // (the host side refuses `hit` for lists beyond 255 objects)
    if (rgb) for (int c = 0; c < 3; c++) rgb[3 * p + c] = col[c];
}

}  // namespace rtgr
