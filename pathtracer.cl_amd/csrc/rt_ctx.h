/*
 * rt_ctx.h — the host runtime's private header: the context behind the C ABI (struct rt_ctx), the
 * owners of its device memory, events and streams, and the few helpers the host translation units
 * share (rt_host.cpp, rt_mesh.cpp, rt_render.cpp, rt_display.cpp).  Host .cpp files only;
 * rt_internal.h stays the host/device interface.
 */
#ifndef RT_CTX_H
#define RT_CTX_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "pathtracer_rt.h"
#include "rt_internal.h"

/* An owning, grow-only device buffer: a pointer and its capacity in elements.  reserve(n) does
   nothing when n <= cap; otherwise it frees the old area, leaves the buffer empty, allocates, and
   records the new capacity only on success (a failed allocation leaves the context consistent).
   Never copies, never shrinks. */
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(DevBuf &&o) noexcept /* (the old area goes with `o`) */
    {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { reset(); }
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        reset();
        const hipError_t e = hipMalloc(&p, n * sizeof(T));
        if (e != hipSuccess) p = nullptr;
        else cap = n;
        return e;
    }
    void reset()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    /* takes over an allocation made elsewhere (the GPU builder's, a grown copy) */
    void adopt(T *q, size_t n)
    {
        reset();
        p = q;
        cap = q ? n : 0;
    }
    operator T *() const { return p; }
};

/* An event / a stream created at first use (create() does nothing after that) and destroyed with
   its owner; moved, never copied. */
template <class H, hipError_t (*Destroy)(H)> struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned &operator=(Owned &&o) noexcept
    {
        std::swap(h, o.h);
        return *this;
    }
    ~Owned()
    {
        if (h) (void)Destroy(h);
    }
    operator H() const { return h; }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { return h ? hipSuccess : hipEventCreateWithFlags(&h, flags); }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create() { return h ? hipSuccess : hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
};

/* glibc random() TYPE_3, the generator behind the reference's rand() (rt_host.cpp) */
struct GlibcRand {
    uint32_t r[34];
    int k = 0;
    void seed(uint32_t s);
    uint32_t next();
};

constexpr size_t kCounterBytes = RT_COUNTER_WORDS * sizeof(unsigned long long);
/* the queue cursors after the counters: the main launch's RT_QHEADS heads RT_QSTRIDE words apart (mq_take),
   then the long chains' and the repairs' one-word cursors on lines of their own */
constexpr size_t kWorkWords = (size_t)RT_QSTRIDE * RT_QHEADS + 64;
static_assert((kCounterBytes + kWorkWords * sizeof(uint32_t)) % sizeof(unsigned long long) == 0, "d_counters is an array of 64-bit words");
#ifndef RT_REPAIR_SLOTS
#define RT_REPAIR_SLOTS 4096u /* repaired pixels with per-sample seeds by slot (8.4 MB at 256 spp) */
#endif

/* the lights' cone split of the host build's shadow tree (rt_mesh.cpp, RT_LIGHT_CONE) */
constexpr bool kLightCone = true;

/* the display-side stages with a kernel time of their own (rt_display.cpp) */
enum RtStage { RT_ST_FEATURES, RT_ST_DENOISE, RT_ST_REPROJECT, RT_ST_MERGE, RT_ST_MOMENTS, RT_ST_VARIANCE, RT_ST_DENOISE_VAR, RT_ST_WARP, RT_ST_TRUST, RT_ST_METER, RT_ST_TONEMAP, RT_ST_WARP_SPH, RT_ST_NOISE, RT_ST_STOP_SELECT, RT_ST_STOP_ORDER, RT_ST_FOLD, RT_ST_BUDGET, RT_ST_PASS_MASK, RT_ST_TILE_LEN, RT_ST_COUNT };

struct rt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    Event ev0, ev1, evm; /* evm: the main kernel's start */
    std::string err;

    /* scene */
    std::vector<rt_sphere> spheres;
    std::vector<rt_sphere> lights;
    DevBuf<rt_sphere> d_spheres, d_lights;

    /* mesh */
    RtBvh bvh;
    DevBuf<float> d_nodes4;     /* 4-wide tree */
    DevBuf<uint32_t> d_nodes4q; /* 4-wide tree, compressed nodes */
    DevBuf<float> d_tris;       /* triangle records, 12 floats each (mesh + camera-ray candidate lists) */
    size_t tris_cap() const { return d_tris.cap / 12; }
    size_t tree_recs = 0;      /* of them the trees' triangle records: n_tris, or 2 n_tris with the shadow tree */
    uint32_t shadow_root = 0;  /* the shadow queries' tree: its root node in d_nodes4q (0: the closest-hit tree) */
    uint32_t n_nodes4_shadow = 0, stack4_all = 0;
    /* the shadow cache (rt_traverse.h ShadowCut): the levels of the shadow queries' tree as node
       ranges (tree_levels), RT_SHADOW_CACHE (0: off) and RT_SHADOW_CACHE_DEPTH (the cut's level,
       -1: the default, kShadowCutDepth) */
    std::vector<std::pair<uint32_t, uint32_t>> shadow_levels;
    bool shadow_cache = true;
    int shadow_cache_depth = -1;
    /* the lights' cone split of the shadow tree (rt_bvh.cpp never_occludes): subtree A's node in
       d_nodes4q (0: none), its triangles, its own levels, and the bits of the (centre, radius) of
       every light the split was made for, 4 words each.  The shadow queries start at A while every
       current light is one of those and the split holds for the records (cone_stale: refitted since —
       a device build with RT_BUILD_OPT_LIGHTS checks the new pose instead, k_refit_cone); else at
       shadow_root (tri_scene) */
    uint32_t cone_root = 0, n_cone = 0;
    std::vector<std::pair<uint32_t, uint32_t>> cone_levels;
    std::vector<uint32_t> cone_lights;
    bool cone_stale = false;
    DevBuf<uint16_t> d_list_code;  /* per pixel: offset in its tile's block << 5 | count - 1 (k_pixel_lists) */
    DevBuf<uint32_t> d_list_tile;  /* per 8x8 tile: first slot of its block of lists */
    DevBuf<uint32_t> d_list_alloc; /* the list area's allocator */
    int pixel_lists = -1; /* RT_PIXEL_LISTS: 0 off, 1 on, unset: on for sampleRate >= 4 (the pre-pass
                             costs about a traversal per pixel: a 1-spp frame does not repay it) */
    size_t list_mb = 4096; /* RT_LIST_MB: device memory of the list area (pixels beyond it take the tree) */
    std::vector<uint32_t> list_key; /* what the lists in the list area were built for (empty: none) */
    uint64_t list_used_last = 0, list_cap_last = 0, list_npx_last = 0; /* the last list build: records taken /
                                                                          given, its pixels */
    std::vector<uint32_t> last_view; /* the previous triangle render's view (camera, mesh, frame, tile) */
    uint32_t n_tris = 0;
    DevBuf<int32_t> d_spill;  /* per-lane stack overflow for the 4-wide traversal */
    DevBuf<uint32_t> d_order; /* pixel-queue tile order (expensive tiles first) */
    DevBuf<uint32_t> d_flags; /* cost probe per pixel (k_probe_cost) */
    RtSchedScratch sched;     /* the device-side schedule (rt_sched.hip) */
    DevBuf<int32_t> d_class;  /* per pixel: -1 mesh, -2 box, >= 0 a long chain's slot (sample-split) */
    size_t split_mb = 16384; /* RT_SPLIT_MB: device memory cap of the sample-split buffers */
    /* sample-split tiles (k_split_seeds -> k_tris chunks -> k_split_finish) */
    int split = -1;                   /* RT_SPLIT: 1 on, 0 off, unset = auto (split_wanted) */
    /* the long chains' seed pass with 4 lanes per query (one lane per query: 8-way tile 24 -> 19 ms
       for the chains); 4 x 4 probe rays per pixel to find them */
    uint32_t seed_width = 0; /* lanes per long chain in the seed pass: 8-64 subtree-parallel (k_chain_seeds), 3 coop_round,
                                1 one lane, 0 by the launch (seed_width_auto) */
    uint32_t split_probe = 4;
    uint32_t split_nch = 16;   /* sample-split: chunk tasks per pixel, about (8 / 13 / 32 no faster, profiles/r05ba) */
    DevBuf<uint32_t> d_split_seed;    /* per pixel and chunk: the seed at the chunk's first sample */
    DevBuf<float> d_split_col;        /* per sample and pixel: its radiance */
    DevBuf<uint32_t> d_split_counter; /* [0]: the seed pass's cursor, [32]: the box pixels' (own line) */
    DevBuf<uint32_t> d_split_box;     /* the box pixels (yl * W + x): their chains run on stream2 */
    DevBuf<uint8_t> d_long_seed;      /* the long chains' seeds by slot, one per RT_LONG_FINE samples (then their hit depths) */
    DevBuf<uint32_t> d_repair_seed;   /* the repaired pixels' seeds by slot (the first RT_REPAIR_SLOTS of them) */
    uint32_t repair_slots = RT_REPAIR_SLOTS; /* RT_REPAIR_SLOTS (env, test knob): repaired pixels with per-sample seeds */
    bool last_hit_depth = false; /* the last sample-split render used split_hit_depth */
    uint32_t n_split_box = 0;
    int split_box_grid = 0;           /* the box pixels' seed-pass grid of the render being launched */
    Stream stream2;                   /* the box pixels' seed pass and chunks, beside the mesh pixels' */
    /* speculated mesh pixels (RT_SPLIT_SPEC, default on): their chunk seeds jumped ahead from the
       frame seeds; a per-pixel mark and the list of the pixels to repair */
    int split_spec = 1;
    DevBuf<uint32_t> d_split_dirty, d_split_repair;
    DevBuf<uint32_t> d_spec_mul;      /* per chunk: the two generators' jump multipliers */
    std::vector<uint32_t> h_spec_mul; /* their host copy (the upload's source; re-uploaded on change) */
    uint64_t spec_mul_key = ~0ull;
    Event ev_split0, ev_box, ev_mesh, ev_fin3;
    Stream stream3;                   /* the clean mesh pixels' in-order sums, beside the repair pass */
    DevBuf<uint32_t> d_halo_rows; /* seed-row halo: row indices */
    DevBuf<uint32_t> d_halo_buf;  /* seed-row halo: staging for host buffers */
    std::vector<uint32_t> order_key; /* what the cached order was computed for */
    bool schedule = true;
    bool schedule_rebuilt = false; /* the last triangle render recomputed the schedule */
    /* measured-cost schedule (whole-pixel frames and sample-split tiles of >= 16 samples per pixel):
       a view's first frame records each pixel's traversal steps (pixel_iter; a split tile's mesh chunk
       tasks), its next frame re-sorts the tiles by them */
    DevBuf<uint32_t> d_pixel_iter; /* two words per pixel (and chunk task) */
    bool iter_recorded = false;  /* this view's costs are in d_pixel_iter */
    bool order_measured = false; /* d_order is sorted by them (once per view: re-sorting again from
                                    the re-sorted frame's costs measured slower, profiles/r05aa) */
    uint32_t iter_nch = 1;       /* chunk tasks per pixel of the recorded frame (1: whole pixels) */
    float mesh_lo[3] = {0, 0, 0}, mesh_hi[3] = {0, 0, 0}; /* the mesh's padded bounds (mesh_bounds) */
    bool mesh_bounds_ok = false;
    rt_render_info info = {};      /* rt_last_render_info */
    bool info_list_pending = false; /* info.list_records / list_pixels_tree still to be read */
    size_t info_list_px = 0;        /* pixels of the render the pending list counts belong to */
    int builder = RT_BUILD_HOST;      /* builder for the next rt_set_mesh */
    int mesh_builder = RT_BUILD_HOST; /* builder of the current mesh */
    uint32_t build_opts = 0;          /* RT_BUILD_OPT_* for the next rt_set_mesh (the device builders) */
    uint32_t mesh_build_opts = 0;     /* ... of the current mesh: a rebuild in rt_update_mesh uses these */
    int collapse = RT_COLLAPSE_GREEDY;      /* RT_COLLAPSE_* for the next rt_set_mesh (the device builders) */
    int mesh_collapse = RT_COLLAPSE_GREEDY; /* ... of the current mesh (a host build: RT_COLLAPSE_SAH) */
    uint64_t mesh_serial = 0;
    /* the moving mesh (rt_update_mesh, rt_refit.hip): the indices of the last rt_set_mesh, on the
       host for a rebuild and on the device for the refit; how that mesh was built; the refit's
       workspace, allocated at the first update (at rt_set_mesh in dynamic mode) and kept until the
       next rt_set_mesh */
    std::vector<int32_t> h_idx;
    DevBuf<int32_t> d_idx;
    DevBuf<float> d_pose; /* the vertices the trees hold: those of the last successful rt_set_mesh /
                             rt_update_mesh, 3 per vertex (rt_mesh_pose, rt_warp_features) */
    uint32_t n_verts = 0;
    bool dynamic = false;       /* the next host build keeps every triangle */
    bool mesh_dynamic = false;  /* the current mesh was built so */
    bool mesh_det_cull = true;  /* ... with normal boxes in its compressed nodes */
    struct Refit {
        bool ready = false;
        DevBuf<float> d_verts;          /* the update's vertices */
        DevBuf<float> d_tbox;           /* padded box per record slot */
        DevBuf<uint8_t> d_hit0;         /* per tree slot: hittable when the tree was built (set by the first update) */
        bool have_hit0 = false;
        DevBuf<float> d_shadow_full;    /* the shadow tree's full-precision nodes */
        DevBuf<uint32_t> d_qscratch;    /* compressed nodes of a tree that has none: the encodability test */
        DevBuf<uint8_t> d_nbox;         /* binary64 normal-box bounds per node (rt_refit_nbox_bytes each) */
        DevBuf<uint32_t> d_res;         /* RT_REFIT_RES_WORDS */
        DevBuf<double> d_part;          /* RT_REFIT_AREA_BLOCKS partial area sums */
        DevBuf<float> d_cone_lights;    /* the lights a device build's cone split was made for (k_refit_cone) */
        DevBuf<RtRefitStep> d_steps;
        std::vector<RtRefitStep> steps; /* deepest level first */
        double area0 = 0.0;             /* the build's own area sum */
        bool have_area0 = false;
        Event ev0, ev1;
    } refit;
    rt_mesh_update_info last_update = {};
    bool have_update = false;
    /* owner-map tiles (rt_tile.stripe_owner): the tile's frame stripes in order, on the device, and a
       serial that changes with them (in the view / schedule keys) */
    std::vector<uint32_t> stripe_map_h;
    DevBuf<uint32_t> d_stripe_map;
    uint32_t stripe_map_serial = 0;
    /* the pilot render of a view's first frame (pilot_order): its seeds, framebuffer and counters +
       queue cursors, apart from the frame's */
    int pilot_sr = 2; /* RT_PILOT (test knob): the pilot's sampleRate, 0 = no pilot (the probe's order) */
    DevBuf<uint32_t> d_pilot_seeds;
    DevBuf<float> d_pilot_out;
    DevBuf<unsigned long long> d_pilot_cnt;
    /* rt_partition_stripes: the last map and what it was computed for */
    std::vector<uint32_t> part_key, part_owner;
    DevBuf<uint32_t> d_part_probe;
    DevBuf<unsigned long long> d_part_cost; /* two words per stripe */

    /* camera state (RayTracer.h:21-29) */
    float view[4][4]; /* viewMatrix, row-major; identity by default (gmtl) */
    float fov = 53.0f; /* RayTracer() default, RayTracer.cpp:18 */
    bool cam_override = false;
    rt_camera cam_explicit;
    bool cam_dirty = true;
    rt_camera cam;
    uint32_t width = 0, height = 0;

    /* settings: RayTracer() defaults (RayTracer.cpp:16-22) */
    uint32_t sample_rate = 8, max_depth = 4;
    int traversal = RT_TRAVERSAL_BVH;
    uint32_t nd_y = 8;
    bool counting = false;

    /* seeds */
    GlibcRand rng;
    uint32_t wpad = 0, hpad = 0;
    bool user_seeds = false;
    DevBuf<uint32_t> d_seeds;

    /* scratch */
    uint32_t *d_work = nullptr;                 /* queue cursors: inside the d_counters allocation, after the counters */
    DevBuf<unsigned long long> d_counters;      /* RT_COUNTER_WORDS counters + guard, then the kWorkWords cursor words */
    unsigned long long *h_counters = nullptr;   /* pinned: the counters (+ the list area's fill) copied back on the render's stream */
    unsigned long long *h_counters_dev = nullptr; /* its device address (mapped): k_counters_out writes it */
    bool counters_zeroed = false;                 /* the last render ended with k_counters_out: no fill needed */
    DevBuf<unsigned long long> d_totals;        /* running totals over renders (k_counters_out; rt_counter_totals) */
    hipStream_t sync_stream = nullptr;          /* the stream of the last render (rt_synchronize waits on it) */
    Event ev_done;                              /* the end of the last render's counter hand-back: a render on another
                                                   stream waits for it (the counters, the queue cursors).  Recorded at
                                                   the render's end on a caller's stream (which may be gone later), and
                                                   only when needed on the context's own (no per-frame record there) */
    DevBuf<float> d_stage;
    rt_counters last = {};
    uint32_t last_long = 0; /* long chains run apart by the last triangle launch (sample-split) */
    bool have_timing = false;
    const float *last_out = nullptr; /* device framebuffer of the last render (rt_read) */
    size_t last_bytes = 0;
    /* persistent-grid size per (traversal kind, counting, kernel form): index (trav * 2 + count) * 3 + form */
    int grid_cache[6 * (RT_TRAV_BVH4Q + 1)] = {};
    /* first-hit features, the display denoiser, the temporal stage and the variance-guided filter
       (rt_features.hip, rt_temporal.hip, rt_filter.hip): scratch and events of their own.
       aux_stream: the stream of the last such call not yet followed by a render (ev_aux: its end) —
       the next render, ray query or probe on another stream waits for it (the spill area, the
       framebuffer the filter reads) */
    DevBuf<float> d_dn_tmp[2];  /* the filter's intermediate passes */
    DevBuf<float> d_var_tmp[2]; /* ... and their variance planes */
    DevBuf<float> d_dn_stage;   /* host buffers' staging */
    DevBuf<uint32_t> d_meter_hist; /* rt_meter_exposure without hist_out: the meter's RT_METER_BINS counts */
    DevBuf<uint32_t> d_noise_hist; /* rt_noise_meter without hist_out, likewise */
    /* adaptive sampling (rt_adaptive.hip).  The stop plane of rt_set_tile_stop: null
       (none set), the caller's device plane, or d_stop_own, the copy of a host plane; the frame it is
       for.  While one is set a triangle render's queue takes d_stop_order, which k_order_stop writes
       before every such launch from d_order (or the identity); d_order itself is never modified. */
    const uint32_t *stop_plane = nullptr;
    uint32_t stop_w = 0, stop_h = 0;
    DevBuf<uint32_t> d_stop_own;
    DevBuf<uint32_t> d_stop_order; /* n_tiles entries, then the live count */
    DevBuf<uint32_t> d_stop_settled; /* rt_tile_stop_select's scratch plane */
    struct StageTime {
        Event e0, e1;
        bool have = false;
    } stage_time[RT_ST_COUNT]; /* each stage's kernels, by RtStage */
    Event ev_aux;
    hipStream_t aux_stream = nullptr;

    /* what no member owns by itself: the schedule's scratch (rt_sched.hip), the pinned counters, the stream */
    ~rt_ctx()
    {
        rt_sched_free(sched);
        if (h_counters) (void)hipHostFree(h_counters);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

static inline std::string *err_of(const rt_ctx *c) { return c ? &const_cast<rt_ctx *>(c)->err : nullptr; }

static inline int fail(rt_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    return code;
}

static inline int hip_fail(rt_ctx *c, hipError_t e, const char *what)
{
    return fail(c, RT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIPCHK(ctx, call)                                                                                              \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess) return hip_fail((ctx), e_, #call);                                                       \
    } while (0)

/* an unsigned environment knob (tuning sweeps), `def` when unset or unparsable */
static inline uint32_t env_u32(const char *name, uint32_t def)
{
    const char *v = getenv(name);
    if (!v || !*v) return def;
    char *end = nullptr;
    const unsigned long x = strtoul(v, &end, 10);
    return (end && *end == 0) ? (uint32_t)x : def;
}

static inline int trav_kind(const rt_ctx *c)
{
    if (c->traversal == RT_TRAVERSAL_LINEAR) return RT_TRAV_LINEAR;
    if (c->traversal == RT_TRAVERSAL_BVH4F || !c->d_nodes4q) return RT_TRAV_BVH4;
    return RT_TRAV_BVH4Q;
}

static inline uint32_t spill_cap(const rt_ctx *c)
{
    /* worst-case stack: the 4-wide tree's stack4 */
    const int k = trav_kind(c);
    const uint32_t need = (k == RT_TRAV_BVH4 || k == RT_TRAV_BVH4Q) ? std::max(c->bvh.stack4, c->stack4_all) : 0u;
    return need > RT_STACK_DEPTH ? need - RT_STACK_DEPTH : 0;
}

static inline const float *trav_nodes(const rt_ctx *c)
{
    const int k = trav_kind(c);
    if (k == RT_TRAV_BVH4Q) return reinterpret_cast<const float *>(c->d_nodes4q.p);
    return k == RT_TRAV_BVH4 ? c->d_nodes4.p : nullptr;
}

static inline int ensure_spill(rt_ctx *c, size_t entries)
{
    HIPCHK(c, c->d_spill.reserve(entries));
    return RT_OK;
}

/* work on `st` that shares buffers with a pending feature / denoise call on another stream: after it */
static inline int wait_aux(rt_ctx *c, hipStream_t st)
{
    if (c->aux_stream && st != c->aux_stream) HIPCHK(c, hipStreamWaitEvent(st, c->ev_aux, 0));
    return RT_OK;
}

/* a render or a display-side call on `st`, another stream than the last render's: ordered after that
   render's counter hand-back (which reads and zeroes the counters and queue cursors) */
static inline int wait_last_render(rt_ctx *c, hipStream_t st)
{
    if (c->sync_stream && st != c->sync_stream) {
        if (c->sync_stream == c->stream) HIPCHK(c, hipEventRecord(c->ev_done, c->stream));
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_done, 0));
    }
    return RT_OK;
}

/* rt_host.cpp: the camera of a frame W pixels wide (RayTracerCL::updateCLCamera), and the seed planes */
rt_camera frame_camera(const rt_ctx *c, uint32_t W);
int ensure_seeds(rt_ctx *c, uint32_t wpad, uint32_t hpad, const uint32_t *src);

#endif /* RT_CTX_H */
