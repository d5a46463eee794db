// rtgr_texture_host.hip — image textures (include/rtgr.h "image textures"): the texel check and the device layout of a load, in Float64 and
// Float32, and the unload — both through the one path of rtgr_tables.hip (retire: a hipGraph captured earlier may still replay the texels;
// rtgr_trim frees them) —, the binds of a call
// into the records the shading kernel reads, the entry points of the shaded trace — the camera frame of rtgr_frame_host.hip without an
// emitting disk — and the sampler hook.  Host code only: the kernels are rtgr_shade.hip's, the mapping and the sampler rtgr_texture.hpp's.
#include "rtgr_internal.hpp"

namespace rtgr {

// Texture ids: a counter of their own, in a range of their own (top bits 0x7…; grid ids carry 0xA…), and never the id of a resident
// unit or table of the context (table_load).
constexpr uint64_t TEXTURE_ID_TAG = 0x7000000000000000ull, TEXTURE_ID_MASK = 0xF000000000000000ull;
static TableIds g_texture_ids{TEXTURE_ID_TAG, TEXTURE_ID_MASK};
constexpr EntryWords SHADED_WORDS = {"rtgr_trace_shaded_*", "shading", true};

int api::texture_load(rtgr_context* ctx, const rtgr_texture_desc* desc, const double* texels, uint64_t* id_out) {
    RESOLVE_CONTEXT();
    if (!desc || !texels || !id_out) return fail(RTGR_ERR_BAD_ARG, "rtgr_texture_load: NULL argument");
    const uint32_t W = desc->width, H = desc->height;
    if (W < 2u || W > RTGR_TEXTURE_MAX_SIDE || H < 2u || H > RTGR_TEXTURE_MAX_SIDE)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_texture_load: width and height must be 2 .. " + std::to_string(RTGR_TEXTURE_MAX_SIDE) + ", got " +
                                      std::to_string(W) + " x " + std::to_string(H));
    if (desc->flags != 0 || desc->pad != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_texture_load: rtgr_texture_desc.flags and .pad must be 0");
    const size_t ntex = (size_t)W * H;
    // every texel finite; the device layout (four scalars per texel) in both scalar types
    std::vector<double> t64(ntex * 4, 0.0);
    std::vector<float> t32(ntex * 4, 0.0f);
    for (int ch = 0; ch < 3; ch++)
        for (size_t q = 0; q < ntex; q++) {
            const double v = texels[ch * ntex + q];
            if (!std::isfinite(v))
                return fail(RTGR_ERR_BAD_ARG, "rtgr_texture_load: texel " + std::to_string(ch * ntex + q) + " (channel " + std::to_string(ch) + ", row " +
                                              std::to_string(q / W) + ", column " + std::to_string(q % W) + ") holds a non-finite value");
            t64[q * 4 + ch] = v;
            t32[q * 4 + ch] = (float)v;
        }
    TextureTable t;
    t.W = W; t.H = H;
    return table_load(c, "rtgr_texture_load", g_texture_ids, &DeviceCtx::textures, t, {{t64.data(), t64.size() * sizeof(double)}},
                      {{t32.data(), t32.size() * sizeof(float)}}, id_out);
}

int api::texture_unload(rtgr_context* ctx, uint64_t id) {
    RESOLVE_CONTEXT();
    const bool found = table_unload(c, &DeviceCtx::textures, id, true);   // (id 0: all of them)
    if (!found) return fail(RTGR_ERR_BAD_ARG, "rtgr_texture_unload: no texture with id " + std::to_string(id) + " is loaded in this context");
    return RTGR_OK;
}

static int filter_check(uint32_t filter) {
    if (filter != RTGR_TEX_NEAREST && filter != RTGR_TEX_BILINEAR)
        return fail(RTGR_ERR_BAD_ARG, "unknown texture filter " + std::to_string(filter) + " (RTGR_TEX_NEAREST = 0, RTGR_TEX_BILINEAR = 1)");
    return RTGR_OK;
}

// the caller's binds into the records the shading kernel reads, for device D and scalar type R (takes D.mu: the texture tables)
template <class R>
int shade_resolve(DeviceCtx& D, const rtgr_scene* scene, const rtgr_shade* shade, ShadeDesc<R>& sd) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!shade) return fail(RTGR_ERR_BAD_ARG, "rtgr_shade is NULL");
    if (shade->flags != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_shade.flags must be 0");
    if (shade->nbind > RTGR_MAX_TEXTURE_BINDS)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_shade.nbind = " + std::to_string(shade->nbind) + ": at most RTGR_MAX_TEXTURE_BINDS (16) binds");
    if (shade->nbind && !shade->bind) return fail(RTGR_ERR_BAD_ARG, "rtgr_shade.bind is NULL");
    if (!(shade->r_escape >= 0.0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_shade.r_escape must be >= 0 (and not NaN)");
    if (scene->nobj > RTGR_OBJECTS_LIMIT || (!scene->objects && scene->nobj > RTGR_MAX_OBJECTS))
        return fail(RTGR_ERR_BAD_ARG, "bad object list: more than RTGR_MAX_OBJECTS objects need rtgr_scene.objects");
    std::memset(&sd, 0, sizeof sd);
    sd.nbind = shade->nbind;
    sd.r_escape = (R)shade->r_escape;
    std::lock_guard<std::mutex> lk(D.mu);
    for (uint32_t k = 0; k < shade->nbind; k++) {
        const rtgr_texture_bind& b = shade->bind[k];
        const std::string who = "rtgr_shade.bind[" + std::to_string(k) + "]";
        int rc;
        if ((rc = filter_check(b.filter))) return fail(rc, who + ": " + last_error_string());
        const TextureTable* t = D.textures.find(b.texture);
        if (!t) return fail(RTGR_ERR_BAD_ARG, who + ": no texture with id " + std::to_string(b.texture) + " is loaded in this context");
        if (b.object > scene->nobj)
            return fail(RTGR_ERR_BAD_ARG, who + ": object " + std::to_string(b.object) + " of a list of " + std::to_string(scene->nobj) + " (1-based; 0 = rays that escape)");
        for (uint32_t q = 0; q < k; q++)
            if (shade->bind[q].object == b.object)
                return fail(RTGR_ERR_BAD_ARG, who + ": " + (b.object ? "object " + std::to_string(b.object) : std::string("the escape")) + " is bound twice");
        DevTexBind<R>& d = sd.bind[k];
        d.tex = (const R*)(sizeof(R) == 8 ? t->d64 : t->d32);
        d.W = t->W; d.H = t->H; d.filter = b.filter; d.object = b.object;
        if (b.object == 0) continue;   // (kind 0: the escape)
        const rtgr_object& o = scene_objects(scene)[b.object - 1];
        if (o.kind == RTGR_SPHERE) { d.kind = RTGR_SPHERE; d.a = (R)o.p[1]; d.b = (R)o.p[2]; d.c = (R)o.p[3]; }
        else if (o.kind == RTGR_DISK) { d.kind = RTGR_DISK; d.a = (R)o.p[1]; d.b = (R)o.p[2]; }
        else
            return fail(RTGR_ERR_BAD_ARG, who + ": object " + std::to_string(b.object) + " is a " + (o.kind == RTGR_PLANE ? "Plane" : o.kind == RTGR_USER_OBJECT ? "user object" : "unknown kind") +
                                          ": textures go on Spheres, Disks and escaping rays");
    }
    return RTGR_OK;
}

int shaded_check(const rtgr_camera* cam, const rtgr_aa* aa, const uint8_t* refined, const rtgr_aa_stats* stats, uint64_t ni, uint64_t nj) {
    if (!cam) return fail(RTGR_ERR_BAD_ARG, "a shaded frame needs a camera (cam is NULL)");
    if (!aa && (refined || stats)) return fail(RTGR_ERR_BAD_ARG, "refined and stats belong to anti-aliasing: they must be NULL when aa is NULL");
    return canvas_check(ni, nj, "a shaded frame");
}

template <class R>
int api::trace_shaded_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                             const rtgr_shade* shade, const rtgr_aa* aa, R* d_rgb, const rtgr_ray_outputs* out, uint8_t* d_refined,
                             rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream) {
    RESOLVE_CONTEXT();
    if (!d_rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    if ((rc = shaded_check(cam, aa, d_refined, stats, ni, nj))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_rgb, &D))) return rc;
    return trace_camera_frame_on<R>(*D, scene, opt, cam, ni, nj, shade, nullptr, aa, d_rgb, out, nullptr, d_refined, ctr, stats, (hipStream_t)stream, SHADED_WORDS);
}

// host pointers: the same call on device 0 of the context, on its staging's compute stream, and the frame copied out
template <class R>
int api::trace_shaded(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                      const rtgr_shade* shade, const rtgr_aa* aa, R* rgb, const rtgr_ray_outputs* out, uint8_t* refined, rtgr_counters* ctr,
                      rtgr_aa_stats* stats) {
    RESOLVE_CONTEXT();
    if (!rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    if ((rc = shaded_check(cam, aa, refined, stats, ni, nj))) return rc;
    if ((rc = check_redshift_outputs(out))) return rc;
    return staged_frame<R>(c, ni * nj, rgb, out, refined, nullptr, [&](DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs* d_out, uint8_t* d_refined, R*, hipStream_t st) {
        return trace_camera_frame_on<R>(D, scene, opt, cam, ni, nj, shade, nullptr, aa, d_rgb, d_out, nullptr, d_refined, ctr, stats, st, SHADED_WORDS);
    });
}

// the sampler at n points, on device 0 of the context (host pointers): rgb goes up too — a "no sample" point keeps its entry
template <class R>
int api::eval_texture(rtgr_context* ctx, uint64_t texture, uint32_t filter, const R* p, uint64_t n, const R* disk_range, R* rgb) {
    RESOLVE_CONTEXT();
    if ((n && !p) || (n && !rgb)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_texture: NULL argument");
    if ((rc = filter_check(filter))) return rc;
    if (n > (1ull << 32)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_texture: at most 2^32 points per call");
    if (disk_range && !(std::isfinite((double)disk_range[0]) && std::isfinite((double)disk_range[1])))
        return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_texture: disk_range = {r_in, r_out} must be finite");
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    TextureTable t;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        const TextureTable* found = D.textures.find(texture);
        if (!found) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_texture: no texture with id " + std::to_string(texture) + " is loaded in this context");
        t = *found;
    }
    if (n == 0) return RTGR_OK;
    const R* d_p = m.in(p, (size_t)n * 3);
    R* d_rgb = m.inout(rgb, (size_t)n * 3);
    if ((rc = m.status())) return rc;
    if ((rc = eval_texture_launch<R>((const R*)(sizeof(R) == 8 ? t.d64 : t.d32), t.W, t.H, filter, disk_range != nullptr, disk_range ? disk_range[0] : R(0),
                                     disk_range ? disk_range[1] : R(0), d_p, n, d_rgb, nullptr)))
        return rc;
    return m.fetch();
}

RTGR_INSTANTIATE_F64_F32(shade_resolve);
RTGR_INSTANTIATE_F64_F32(api::trace_shaded_device);
RTGR_INSTANTIATE_F64_F32(api::trace_shaded);
RTGR_INSTANTIATE_F64_F32(api::eval_texture);

}  // namespace rtgr
