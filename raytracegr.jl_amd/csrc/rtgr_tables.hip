// rtgr_tables.hip — what a context keeps resident on its devices for the kernels to read, under ONE lifetime rule (rtgr_host.hpp: Resident,
// ObjectTable).  Written once here, for grid metrics (rtgr_grid.hip) and image textures (rtgr_texture_host.hip) alike: the draw of an id, the
// upload of a table's Float64 and Float32 images to every device with roll-back, its publication, the unload, the counts of the test hooks;
// and the tables of long object lists, found by content (convert_scene, rtgr_scene_host.hip).  Host code only.
#include "rtgr_internal.hpp"

namespace rtgr {

void free_all(const std::vector<void*>& ptrs) {
    for (void* p : ptrs) if (p) (void)hipFree(p);
}

// ---- tables named by an id -----------------------------------------------------------------------------------------------------------
template <class T>
int table_load(rtgr_context* c, const char* who, TableIds& ids, Resident<T> DeviceCtx::*kind, T t, const TableImage& image64,
               const TableImage& image32, uint64_t* id_out) {
    std::lock_guard<std::mutex> load_lock(c->modules_mu);   // (units and tables of every kind are loaded / unloaded under the same lock)
    // an id of the kind's own range that no unit and no resident table of any kind on any device carries
    for (;;) {
        t.id = ids.tag | (ids.next.fetch_add(1) & ~ids.mask);
        bool taken = false;
        for (auto& d : c->devs) {
            std::lock_guard<std::mutex> lk(d->mu);
            taken = taken || d->find_module(t.id) || d->grids.find(t.id) || d->textures.find(t.id);
        }
        if (!taken) break;
    }
    // allocate and upload everywhere first; the table becomes visible to calls only when every device has its copy
    std::vector<T> made(c->devs.size(), t);
    auto release = [&]() {
        for (size_t k = 0; k < made.size(); k++) {
            DeviceGuard guard(c->devs[k]->dev);
            free_all({made[k].d64, made[k].d32});
        }
    };
    auto upload = [](void** dev, const TableImage& image) {
        size_t bytes = 0;
        for (auto& seg : image) bytes += seg.bytes;
        hipError_t e = hipMalloc(dev, bytes);
        size_t at = 0;
        for (auto& seg : image) {
            if (e == hipSuccess) e = hipMemcpy((char*)*dev + at, seg.p, seg.bytes, hipMemcpyHostToDevice);
            at += seg.bytes;
        }
        return e;
    };
    for (size_t k = 0; k < c->devs.size(); k++) {
        DeviceGuard guard(c->devs[k]->dev);
        if (!guard.ok) { release(); return fail(RTGR_ERR_HIP, "hipSetDevice failed"); }
        hipError_t e = upload(&made[k].d64, image64);
        if (e == hipSuccess) e = upload(&made[k].d32, image32);
        if (e != hipSuccess) {
            release();
            return fail(RTGR_ERR_HIP, std::string(who) + ": upload to device " + std::to_string(k) + ": " + hipGetErrorString(e));
        }
    }
    for (size_t k = 0; k < c->devs.size(); k++) {
        std::lock_guard<std::mutex> lk(c->devs[k]->mu);
        (c->devs[k].get()->*kind).publish(made[k]);
    }
    *id_out = t.id;
    return RTGR_OK;
}
template int table_load(rtgr_context*, const char*, TableIds&, Resident<GridTable> DeviceCtx::*, GridTable, const TableImage&, const TableImage&, uint64_t*);
template int table_load(rtgr_context*, const char*, TableIds&, Resident<TextureTable> DeviceCtx::*, TextureTable, const TableImage&, const TableImage&, uint64_t*);

template <class T>
bool table_unload(rtgr_context* c, Resident<T> DeviceCtx::*kind, uint64_t id, bool zero_means_all) {
    std::lock_guard<std::mutex> load_lock(c->modules_mu);
    bool found = false;
    for (auto& d : c->devs) {
        std::lock_guard<std::mutex> lk(d->mu);
        found = (d.get()->*kind).retire(id, zero_means_all) || found;   // (not freed: a captured hipGraph may replay it until rtgr_trim)
    }
    return found;
}
template bool table_unload(rtgr_context*, Resident<GridTable> DeviceCtx::*, uint64_t, bool);
template bool table_unload(rtgr_context*, Resident<TextureTable> DeviceCtx::*, uint64_t, bool);

// ---- the tables of long object lists ---------------------------------------------------------------------------------------------------
constexpr size_t OBJECT_TABLES_MAX = 512;
constexpr size_t OBJECT_TABLES_BYTES = (size_t)1 << 30;

// The device table of the objects beyond the argument block (ObjectTable, rtgr_host.hpp): found by content, uploaded on first sight.
int object_table(DeviceCtx& D, const std::vector<char>& content, hipStream_t st, const void** dev) {
    const uint64_t key = fnv1a(content);
    const bool capturing = st && stream_capturing(st);
    auto range = D.object_tables.equal_range(key);
    for (auto it = range.first; it != range.second; ++it)
        if (it->second.content == content) {
            if (capturing) it->second.kept = true;   // the graph will replay it: from now on it goes with rtgr_trim / rtgr_destroy only
            *dev = it->second.dev;
            return RTGR_OK;
        }
    if (capturing)
        return fail(RTGR_ERR_BAD_ARG, "a scene of more than RTGR_MAX_OBJECTS objects is seen for the first time while the stream is being captured "
                                      "(its object table must be uploaded): trace the scene once before hipStreamBeginCapture");
    if (D.object_tables.size() >= OBJECT_TABLES_MAX || D.object_table_bytes + content.size() > OBJECT_TABLES_BYTES) {
        // a caller that animates a long list: start over with what no graph holds (nothing in flight may read a freed table)
        HIP_TRY(hipDeviceSynchronize());
        for (auto it = D.object_tables.begin(); it != D.object_tables.end();) {
            if (it->second.kept) { ++it; continue; }
            (void)hipFree(it->second.dev);
            D.object_table_bytes -= it->second.content.size();
            it = D.object_tables.erase(it);
        }
    }
    ObjectTable t;
    HIP_TRY(hipMalloc(&t.dev, content.size()));
    const hipError_t e = hipMemcpy(t.dev, content.data(), content.size(), hipMemcpyHostToDevice);   // blocking: complete before any launch
    if (e != hipSuccess) { (void)hipFree(t.dev); return fail(RTGR_ERR_HIP, std::string("hipMemcpy(object table): ") + hipGetErrorString(e)); }
    t.content = content;
    D.object_table_bytes += content.size();
    *dev = t.dev;
    D.object_tables.emplace(key, std::move(t));
    return RTGR_OK;
}

std::vector<void*> drain_object_tables(DeviceCtx& d) {
    std::vector<void*> out;
    for (auto& kv : d.object_tables) out.push_back(kv.second.dev);
    d.object_tables.clear();
    d.object_table_bytes = 0;
    return out;
}

// what a hook below reports of device `index`, read under its lock
static int count_tables(rtgr_context* ctx, int index, uint32_t* a, uint32_t* b, std::pair<size_t, size_t> (*count)(const DeviceCtx&)) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if (index < 0 || (size_t)index >= c->devs.size() || !a || !b) return fail(RTGR_ERR_BAD_ARG, "bad argument");
    DeviceCtx& d = *c->devs[(size_t)index];
    std::lock_guard<std::mutex> lk(d.mu);
    const auto n = count(d);
    *a = (uint32_t)n.first;
    *b = (uint32_t)n.second;
    return RTGR_OK;
}

}  // namespace rtgr

// Test hooks, not part of include/rtgr.h (tests/test_grid_metric.py, test_textures.py, test_gpu_context.py): the tables on device `index`
// of the context — grids and textures: resident and retired (unloaded, waiting for rtgr_trim); object lists: all, and those a graph holds.
extern "C" int rtgr_testhook_grid_tables(rtgr_context* ctx, int index, uint32_t* resident, uint32_t* retired) {
    return rtgr::count_tables(ctx, index, resident, retired, [](const rtgr::DeviceCtx& d) { return std::make_pair(d.grids.n_resident(), d.grids.n_retired()); });
}
extern "C" int rtgr_testhook_texture_tables(rtgr_context* ctx, int index, uint32_t* resident, uint32_t* retired) {
    return rtgr::count_tables(ctx, index, resident, retired, [](const rtgr::DeviceCtx& d) { return std::make_pair(d.textures.n_resident(), d.textures.n_retired()); });
}
extern "C" int rtgr_testhook_object_tables(rtgr_context* ctx, int index, uint32_t* resident, uint32_t* kept) {
    return rtgr::count_tables(ctx, index, resident, kept, [](const rtgr::DeviceCtx& d) {
        size_t held = 0;
        for (auto& kv : d.object_tables) held += kv.second.kept;
        return std::make_pair(d.object_tables.size(), held);
    });
}
