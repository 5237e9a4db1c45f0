/*
 * rt_render.cpp — the renders of a context (librtmi.so host runtime): the schedule of the
 * triangle kernel's launch (grid, tile order, sample split, speculation, pilot, candidate lists),
 * the launches of the render kernels (rt_tris.hip, rt_split.hip, rt_lists.hip, rt_sched.hip,
 * rt_spheres.hip), the stripe partition, the counters, the render info and the kernel times, the
 * seed-row halo, rt_read and rt_trace_rays.
 */
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "rt_ctx.h"

namespace {

/* Scheduling constants of the triangle kernel, each swept on the dragon frame (DESIGN.md §5;
   results are independent of all of them):
     kProbeN    cost-probe rays per pixel, kProbeN x kProbeN;
     kFetchK    completed queries that end a wave's stepping round (12 / 16 / 20 / 24 / 32 / 40:
                166.8 / 163.9 / 163.0 / 162.3 / 163.9 / 168.2 ms); the same for waves holding
                box pixels (8 / 16 / 24 within 0.5 %);
     kFetchFrac the stepping round also ends at ceil(live lanes x kFetchFrac / 64) completed
                queries (r02 A/B: full frame 162.8 -> 160.6 ms, slowest 8-way tile 219 -> 107 ms). */
constexpr uint32_t kProbeN = 2;
/* a 1-spp frame traces fewer rays than a 2x2 probe would: one probe ray per pixel there (bunny
   class 1024^2 at 1 spp: a camera move cost 2.2 ms against a 1.0 ms frame with the 2x2 probe) */
uint32_t probe_n(uint32_t sample_rate) { return sample_rate >= 2 ? kProbeN : 1u; }
#ifndef RT_FETCH_K
#define RT_FETCH_K 24
#endif
/* the long chains' and the repairs' queue cursors, after the main launch's heads (kWorkWords, rt_ctx.h) */
constexpr uint32_t kWorkBox = RT_QSTRIDE * RT_QHEADS, kWorkRepair = RT_QSTRIDE * RT_QHEADS + 32;
#ifndef RT_LONG_FINE
#define RT_LONG_FINE 1 /* samples per stored seed (and per chunk task) of the subtree-parallel long chains */
#endif
#ifndef RT_REPAIR_WIDTH
#define RT_REPAIR_WIDTH 64u /* lanes per repaired chain: its hit samples in runs of 63 */
#endif
#ifndef RT_QUEUE_BATCH
#define RT_QUEUE_BATCH 64
#endif
#ifndef RT_BOX_GRID_DIV
#define RT_BOX_GRID_DIV 4 /* the long chains' seed pass takes at most 1/RT_BOX_GRID_DIV of the persistent grid */
#endif
#ifndef RT_SEED_GRID_ITEMS
#define RT_SEED_GRID_ITEMS 1
#endif
constexpr uint32_t kFetchK = RT_FETCH_K;
constexpr uint64_t kShortFrameSamplesPerLane = 8; /* below: a short frame (fewer blocks per CU) */
constexpr int kShortFrameBlocksPerCU = 3;
/* the pilot render (pilot_order) only for frames of at least this many samples per pixel: its 4 spp
   are 1.6 % of a 256-spp frame, but a quarter of the Lucy class's 16-spp frame (133 against 506 ms,
   profiles/r06f), which keeps the probe's order */
constexpr uint32_t kPilotMinSpp = 64;
constexpr uint32_t kFetchFrac = 24;
/* the shadow cache's default cut: the tree level whose subtrees hold one pixel's bundle of shadow
   rays best (dragon class, cuts 4 / 5 / 6: 72.6 / 71.0 / 72.4 ms against 75.6 without) */
constexpr size_t kShadowCutDepth = 5;
/* the inline list resolve of k_tris's phase B: the records of a pixel's candidate
   list its camera rays are tested against where they are made (RT_INLINE_LIST, 0 to RT_INLINE_MAX;
   0: none), and the passes of an iteration's path advance after the first that may still do so
   (RT_INLINE_CHAIN); scheduling only.  Dragon frame, K 0 / 1 / 2 / 3 / 4 without chained rounds:
   71.1 / 77.2 / 69.4 / 70.4 / 71.7 ms, K 2 with one / two chained rounds 74.7 / 79.9.
   Short frames (they lose with it) and sample-split launches (not measured with it) keep K 0 unless
   RT_INLINE_LIST is set */
constexpr uint32_t kInlineList = 2;
constexpr uint32_t kInlineChain = 0;

/* Grow the triangle buffer to `records` 48-B records, keeping the first `keep` (the mesh's). */
int ensure_tris_capacity(rt_ctx *c, size_t records, size_t keep, hipStream_t st, bool shrink = false)
{
    /* grows to `records`; with `shrink`, also gives back an area more than twice the need */
    if (records <= c->tris_cap() && !(shrink && c->tris_cap() > keep + 2 * (records - keep) + (1u << 20))) return RT_OK;
    float *nt = nullptr;
    HIPCHK(c, hipMalloc(&nt, records * 48));
    hipError_t e = hipMemcpyAsync(nt, c->d_tris, keep * 48, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(nt);
        return hip_fail(c, e, "triangle buffer copy");
    }
    c->d_tris.adopt(nt, records * 12);
    c->list_key.clear(); /* only the mesh's records were carried over */
    return RT_OK;
}

int grid_blocks(rt_ctx *c, int trav, bool count, int form, int *out)
{
    const int key = (trav * 2 + (count ? 1 : 0)) * 3 + form;
    if (key < 0 || key >= (int)(sizeof(c->grid_cache) / sizeof(c->grid_cache[0])))
        return fail(c, RT_ERR_ARG, "unknown traversal kind");
    if (!c->grid_cache[key]) {
        int b = 0;
        const int e = rt_tris_grid_blocks(c->device, trav, count, form, &b);
        if (e) return hip_fail(c, (hipError_t)e, "occupancy query");
        c->grid_cache[key] = b;
    }
    *out = c->grid_cache[key];
    return RT_OK;
}

/* Sample-split tiles (RT_SPLIT): when a launch has fewer pixels than about two
   per resident lane — a multi-GPU tile of a many-sample frame — every lane holds one pixel
   from the start and the launch lasts as long as its slowest pixel's serial sample chain.
   Splitting each pixel's samples into chunks (seeded by a closest-hit-only pass) turns it back
   into a queue of many short tasks.  Automatic below two pixels per lane at sampleRate >= 4
   (dragon class, 1920x1080 at 256 spp, one rank's row-stripe tile: 4-way 42.1 -> 35.6 ms, 8-way
   29.2 -> 24.8 ms; 2-way 59.3 -> 68.3 and the whole frame 96.5 -> 127.4 ms would lose:
   profiles/r03v). */
bool split_wanted(const rt_ctx *c, uint64_t npx, uint64_t lanes)
{
    if (c->sample_rate < 2) return false;
    return c->split == 1 || (c->split < 0 && npx < 2 * lanes && c->sample_rate >= 4);
}

/* The long chains' seed-pass form for a sample-split launch: below 1.2 pixels per resident lane
   (the 8-way tile of the 1920x1080 frame: 0.8) the chains are the tile's critical path and take
   8 subtree-parallel lanes each (k_chain_seeds: 8-way tile 18.5 -> 16.4 ms); above it (the 4-way
   tile: 1.6) the chunks' throughput is, and the 4-lane cooperative pass, lighter on the chip,
   wins (4-way tile 32.5 -> 30.1 ms; profiles/r04t). */
uint32_t seed_width_auto(uint64_t npx, uint64_t lanes) { return npx * 5 < lanes * 6 ? 8u : (uint32_t)RT_SEED_COOP4; }

/* Sample-split buffers: per pixel (nch + 1) seed pairs, per sample and pixel an RGB radiance. */
int ensure_split(rt_ctx *c, size_t seed_bytes, size_t col_bytes)
{
    HIPCHK(c, c->d_split_seed.reserve(seed_bytes / sizeof(uint32_t)));
    HIPCHK(c, c->d_split_col.reserve(col_bytes / sizeof(float)));
    HIPCHK(c, c->d_split_counter.reserve(64));
    HIPCHK(c, c->stream2.create());
    HIPCHK(c, c->ev_split0.create(hipEventDisableTiming));
    HIPCHK(c, c->ev_box.create(hipEventDisableTiming));
    HIPCHK(c, c->stream3.create());
    HIPCHK(c, c->ev_mesh.create(hipEventDisableTiming));
    HIPCHK(c, c->ev_fin3.create(hipEventDisableTiming));
    return RT_OK;
}

/* The long chains' seed-pass grid: one chain per group of `width` lanes, at most a quarter of
   the full grid (further chains queue behind the first) — subtree-parallel chains at most three
   quarters, so the mesh pixels' chunk launch beside it keeps a quarter of the grid (a tile with
   tens of thousands of chains left it one block: RT_SEED_WIDTH=8 on the 2-way tile ran for
   seconds, profiles/r05bc; 77 ms with the cap, r05bf); full_grid 0: unbounded. */
int split_box_blocks(const rt_ctx *c, uint32_t width, int full_grid)
{
    const uint32_t per_wave = 64u / std::max(1u, width == RT_SEED_COOP4 ? 4u : width);
    int n = (int)((c->n_split_box + per_wave * 4u - 1u) / (per_wave * 4u));
    /* subtree-parallel chains (width >= 8) all run at once where they fit: each is the critical path */
    if (full_grid > 0) n = std::min(n, std::max(1, width >= 8 ? full_grid * 3 / 4 : full_grid / RT_BOX_GRID_DIV));
    return n;
}

/* Speculated mesh pixels: every mesh pixel's sample draws 2 + 2 x lights random
   numbers, so chunk c starts c x chunk x D draws after the frame seed; per chunk the jump
   multipliers A^(c chunk D) mod A 2^16 - 1 of the two MWC generators (rng.h:9-47), computed here
   and uploaded when they change; the per-pixel marks are cleared for the render. */
uint32_t powmod(uint64_t a, uint64_t e, uint64_t m)
{
    uint64_t r = 1 % m;
    a %= m;
    while (e) {
        if (e & 1u) r = r * a % m;
        a = a * a % m;
        e >>= 1;
    }
    return (uint32_t)r;
}

int spec_setup(rt_ctx *c, RtTriLaunch &a, size_t npx, hipStream_t st)
{
    const uint32_t draws = 2u + 2u * (uint32_t)c->lights.size();
    const uint64_t key = (uint64_t)a.split_chunks << 40 | (uint64_t)a.split_chunk << 20 | draws;
    HIPCHK(c, c->d_spec_mul.reserve(4 * 64));
    if (a.split_chunks > 64) return fail(c, RT_ERR_ARG, "speculated split: more than 64 chunks");
    if (key != c->spec_mul_key) {
        c->h_spec_mul.assign(4 * 64, 1u);
        for (uint32_t ch = 0; ch < a.split_chunks; ++ch) {
            const uint64_t k = (uint64_t)ch * a.split_chunk * draws;
            c->h_spec_mul[2 * ch] = powmod(36969u, k, 36969ull * 65536u - 1u);
            c->h_spec_mul[2 * ch + 1] = powmod(18000u, k, 18000ull * 65536u - 1u);
        }
        for (uint32_t j = 0; j < 64; ++j) { /* the repair's runs: lane j's sample is j x D draws on */
            c->h_spec_mul[128 + 2 * j] = powmod(36969u, (uint64_t)j * draws, 36969ull * 65536u - 1u);
            c->h_spec_mul[128 + 2 * j + 1] = powmod(18000u, (uint64_t)j * draws, 18000ull * 65536u - 1u);
        }
        /* on the render stream, after the previous frame's chunk tasks and repair pass (which read
           the multipliers: split_render ends with the render stream waiting on the other two); the
           wait keeps the host copy alive until the upload is done (a rare event: the key changes
           with the chunking or the light count) */
        HIPCHK(c, hipMemcpyAsync(c->d_spec_mul, c->h_spec_mul.data(), 4 * 64 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->spec_mul_key = key;
    }
    HIPCHK(c, c->d_split_dirty.reserve(npx));
    HIPCHK(c, c->d_split_repair.reserve(npx));
    HIPCHK(c, hipMemsetAsync(c->d_split_dirty, 0xff, npx * sizeof(uint32_t), st));
    a.split_spec = 1;
    a.split_spec_draws = draws;
    a.split_spec_mul = c->d_spec_mul;
    a.split_run_mul = c->d_spec_mul + 128;
    a.split_dirty = c->d_split_dirty;
    a.split_repair = c->d_split_repair;
    return RT_OK;
}

/* The long chains' mesh-hit depths (split_hit_depth): their subtree-parallel seed pass answers, for
   every segment of every sample, whether its closest-hit query accepts a triangle — the same answer
   the chunk task's traversal would give (the seeds depend on it) — and stores the depth of the one
   that does (a path ends at its mesh hit, rtcommon.h:411-421); a chunk task then answers the box
   segments above it without a traversal.  One sample per task (the depth is read at the take), and
   depths in a byte.  Not for the repair pass: its chains are mesh pixels, whose paths meet the mesh
   at the camera ray. */
bool hit_depth_on(const rt_ctx *c, const RtTriLaunch &t)
{
    (void)c;
    return (t.split_coop >= 8 || t.split_coop == RT_SEED_COOP4) && !t.split_restart && t.split_chunk == 1u && t.max_depth < 255u;
}

/* A sample-split render: the box pixels' seed pass, their chunks and their in-order sums on
   stream2, beside the mesh pixels' seed pass (none when speculated) and chunks on the render
   stream (the box pixels' chains are the long ones: they overlap the rest of the frame instead
   of preceding it); the clean mesh pixels' sums on stream3 beside the repair pass, then the
   repaired pixels' sums.  Each stream has its own queue cursors and its own part of the spill area. */
int split_render(rt_ctx *c, const RtTriLaunch &a, int blocks, hipStream_t st)
{
    const uint32_t n_box = a.split_which == RT_SPLIT_MESH ? a.split_n_box : 0u;
    if (n_box) {
        RtTriLaunch b = a;
        b.split_which = RT_SPLIT_BOX;
        b.pixel_iter = nullptr; /* the measured costs: the mesh pixels' chunk tasks only */
        b.split_counter = a.split_counter + 32;
        b.work_counter = a.work_counter + kWorkBox;
        b.spill = a.spill + (size_t)std::max<int>(blocks, (int)a.split_seed_blocks) * RT_BLOCK * a.spill_cap;
        b.split_gpw = 0;
        b.split_seed_blocks = (uint32_t)std::max(1, c->split_box_grid);
        b.split_chunk = a.split_fine; /* the long chains' chunks: one stored seed each */
        b.split_chunks = (a.sample_rate * a.sample_rate + b.split_chunk - 1u) / b.split_chunk;
        HIPCHK(c, hipEventRecord(c->ev_split0, st));
        HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_split0, 0));
        if (a.split_coop >= 8 || a.split_coop == RT_SEED_COOP4) {
            /* the long chains' pass (subtree-parallel or cooperative) stores a chain's seed every
               RT_LONG_FINE samples into a buffer of its own, by slot, and each sample's mesh-hit
               depth: their chunk tasks are that short, so the long chains' last chunks (box paths,
               the costliest samples) do not trail the tile */
            const uint32_t spp = a.sample_rate * a.sample_rate;
            b.split_fine = RT_LONG_FINE;
            b.split_chunk = RT_LONG_FINE;
            b.split_chunks = (spp + RT_LONG_FINE - 1u) / RT_LONG_FINE;
            b.split_nseed = b.split_chunks + 1u;
            const size_t seed_bytes = (size_t)n_box * b.split_nseed * 8u;
            const bool hd = hit_depth_on(c, b);
            const size_t bytes = seed_bytes + (hd ? (size_t)n_box * spp : 0u);
            HIPCHK(c, c->d_long_seed.reserve(bytes));
            b.split_seed = reinterpret_cast<uint32_t *>(c->d_long_seed.p);
            b.split_seed_slot = 1;
            b.split_hit_depth = hd ? c->d_long_seed + seed_bytes : nullptr;
            c->last_hit_depth = hd;
        }
        const int chunk_grid = (int)std::min<uint64_t>((uint64_t)blocks, ((uint64_t)n_box * b.split_chunks + RT_BLOCK - 1) / RT_BLOCK);
        int e = rt_launch_split_seeds(b, c->stream2);
        if (!e) e = rt_launch_tris(b, RT_TRAV_BVH4Q, c->counting, std::max(1, chunk_grid), c->stream2);
        RtTriLaunch f = b; /* the long chains' in-order sums, as soon as their chunks are done */
        f.finish_part = RT_FIN_LIST;
        if (!e) e = rt_launch_split_finish(f, c->stream2);
        if (e) return hip_fail(c, (hipError_t)e, "box-pixel split launches");
        HIPCHK(c, hipEventRecord(c->ev_box, c->stream2));
    }
    RtTriLaunch m = a; /* the mesh pixels' seed pass: short chains, one lane each */
    m.split_coop = 0;
    int e = a.split_spec ? 0 : rt_launch_split_seeds(m, st); /* speculated: no seed pass */
    if (!e) e = rt_launch_tris(m, RT_TRAV_BVH4Q, c->counting, blocks, st);
    if (e) return e;
    if (n_box) { /* the mesh pixels no chunk of which missed: summed on stream3, beside the repair pass */
        HIPCHK(c, hipEventRecord(c->ev_mesh, st));
        HIPCHK(c, hipStreamWaitEvent(c->stream3, c->ev_mesh, 0));
        RtTriLaunch f = a;
        f.finish_part = RT_FIN_MESH;
        e = rt_launch_split_finish(f, c->stream3);
        if (e) return hip_fail(c, (hipError_t)e, "mesh-pixel sums");
        HIPCHK(c, hipEventRecord(c->ev_fin3, c->stream3));
    }
    if (!n_box) return rt_launch_split_finish(a, st);
    if (a.split_spec) {
        /* the repair pass: the speculated pixels a camera ray of which missed the mesh, as long
           chains from their first missed chunk (seed pass, chunks, sums), their count read on
           the device (usually none: the grids find no item and end).  With the subtree-parallel
           pass the first RT_REPAIR_SLOTS of them store a seed per sample by slot, so their chunk
           tasks are single samples; any beyond take the per-pixel seeds */
        RtTriLaunch r = a;
        r.split_spec = 0;
        r.pixel_iter = nullptr;
        r.split_which = RT_SPLIT_BOX;
        r.split_box = a.split_repair;
        r.split_n_box = 0;
        r.split_n_dev = reinterpret_cast<const uint32_t *>(a.counters + RT_CNT_REPAIR);
        r.split_counter = a.split_counter + 48;
        r.work_counter = a.work_counter + kWorkRepair;
        r.split_gpw = 0;
        r.split_seed_blocks = 16u * RT_REPAIR_WIDTH / 16u; /* RT_REPAIR_WIDTH blocks of 4 waves, one chain per wave
                                                                at width 64: up to 256 chains at once */
        r.split_chunk = a.split_fine;
        r.split_chunks = (a.sample_rate * a.sample_rate + r.split_chunk - 1u) / r.split_chunk;
        r.split_restart = a.split_dirty; /* each chain from its first missed chunk on */
        r.split_restart_chunk = a.split_chunk;
        r.finish_part = RT_FIN_LIST;
        /* the runs form also where the long chains take the cooperative pass (the 4-way tile: the
           repair 2.7 -> 2.1 ms at the end of the mesh pixels' stream, the tile 28.83 -> 28.39 ms, profiles/r05bg, r05bh) */
        {
            const uint32_t spp = a.sample_rate * a.sample_rate;
            r.split_coop = RT_REPAIR_WIDTH; /* runs of width - 1 hit samples (k_chain_seeds<width, true>) */
            RtTriLaunch s = r;
            s.split_fine = RT_LONG_FINE;
            s.split_chunk = RT_LONG_FINE;
            s.split_chunks = (spp + RT_LONG_FINE - 1u) / RT_LONG_FINE;
            s.split_nseed = s.split_chunks + 1u;
            s.split_item_cap = c->repair_slots;
            const size_t bytes = (size_t)c->repair_slots * s.split_nseed * 8u;
            HIPCHK(c, c->d_repair_seed.reserve(bytes / sizeof(uint32_t)));
            s.split_seed = c->d_repair_seed;
            s.split_seed_slot = 1;
            e = rt_launch_split_seeds(s, st);
            if (!e) e = rt_launch_tris(s, RT_TRAV_BVH4Q, c->counting, 128, st);
            if (!e) e = rt_launch_split_finish(s, st);
            if (e) return hip_fail(c, (hipError_t)e, "repair launches");
            r.split_item_base = c->repair_slots; /* the rest, if any */
        }
        e = rt_launch_split_seeds(r, st);
        if (!e) e = rt_launch_tris(r, RT_TRAV_BVH4Q, c->counting, 64, st);
        if (!e) e = rt_launch_split_finish(r, st);
        if (e) return hip_fail(c, (hipError_t)e, "repair launches");
    }
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_box, 0));
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_fin3, 0));
    return RT_OK;
}

/* LPT scheduling of the pixel queue.  The reference's per-pixel cost is set by its paths: a
   camera ray that hits the mesh ends after one shadow query per light (rtcommon.h:411-421),
   one that misses bounces off the box up to maxDepth+1 times with shadow queries at each
   (rtcommon.h:425-461), and each query costs its traversal steps.  A probe (k_probe_cost)
   traces a grid of camera rays per pixel (2x2; 4x4 for a sample-split render) and, on mesh
   hits, their shadow rays toward the light centres with the real traversal, counting steps.
   From it the device computes the tile costs, the LPT order (most expensive 8x8 tiles first,
   so the launch does not end on a tail of long pixels) and the pixel classes (rt_sched.hip).
   A sample-split render (split_wanted) also takes its long chains from it — the box pixels
   (some probe ray missed the mesh) and the mesh pixels whose probe took more than 96 steps per
   ray — at the price of one 4-byte read (their count, to size the slot list).  Scheduling
   only: every pixel's result is independent of when and where it is rendered.  Cached until
   camera, mesh, traversal, frame, tile or path parameters change. */
int tile_order(rt_ctx *c, const RtTriLaunch &a, int blocks, hipStream_t st)
{
    const uint32_t W = a.W, hl = a.Hl;
    /* everything the order and the pixel classes depend on — including the traversal (only
       the compressed tree is probed: a key without it would hand a BVH4F / linear launch stale
       classes) */
    const uintptr_t np = reinterpret_cast<uintptr_t>(a.nodes);
    std::vector<uint32_t> key = {a.W, a.H, hl, a.stripe, a.n_ranks, a.rank, a.map_key, c->max_depth, (uint32_t)c->lights.size(),
                                 (uint32_t)c->mesh_serial, (uint32_t)(c->mesh_serial >> 32), (uint32_t)blocks,
                                 c->sample_rate, (uint32_t)(c->split + 1) | (uint32_t)c->split_spec << 8,
                                 (uint32_t)trav_kind(c), (uint32_t)np,
                                 (uint32_t)((uint64_t)np >> 32)};
    const uint32_t *cb = reinterpret_cast<const uint32_t *>(&c->cam);
    key.insert(key.end(), cb, cb + sizeof(rt_camera) / 4);
    const uint32_t n_t = ((W + 7) / 8) * ((hl + 7) / 8);
    c->schedule_rebuilt = false;
    if (key == c->order_key) {
        if (c->iter_recorded && !c->order_measured && c->d_order) {
            /* the view's second frame: its tiles by the first frame's measured costs (the probe's
               few rays miss where the samples' shadow rays are long: dragon frame) */
            const int e = rt_sched_order_measured(c->sched, c->d_pixel_iter, W, hl, c->iter_nch, c->d_order, st);
            if (e) return hip_fail(c, (hipError_t)e, "measured tile order");
            c->order_measured = true;
        }
        return RT_OK;
    }
    c->order_key.clear();
    c->iter_recorded = false;
    c->order_measured = false;
    c->n_split_box = 0;
    if (trav_kind(c) != RT_TRAV_BVH4Q || a.nodes != reinterpret_cast<const float *>(c->d_nodes4q.p)) {
        /* the probe walks the compressed tree with its spill layout: other traversal kinds
           (measurement variants) keep the row-major queue and no classes */
        c->d_order.reset();
        c->order_key = key;
        return RT_OK;
    }
    const size_t npx = (size_t)W * hl;
    HIPCHK(c, c->d_flags.reserve(npx));
    HIPCHK(c, c->d_class.reserve(npx));
    HIPCHK(c, c->d_order.reserve(n_t));
    const bool split = split_wanted(c, npx, (uint64_t)blocks * RT_BLOCK);
    RtTriLaunch pa = a;
    pa.probe_n = split && c->sample_rate >= 4 ? c->split_probe : probe_n(c->sample_rate);
    /* a whole-pixel frame that a pilot render will order (pilot_order): the probe only classes the
       pixels (box pixels: the issue priority), one ray each */
    const bool pilot_next = !split && c->pilot_sr > 0 && c->sample_rate * c->sample_rate >= kPilotMinSpp && !c->counting;
    if (pilot_next) pa.probe_n = 1;
    const uint32_t pn2 = pa.probe_n * pa.probe_n;
    int e = rt_launch_probe_cost(pa, blocks, c->d_flags, st);
    if (e) return hip_fail(c, (hipError_t)e, "probe launch");
    /* (the probe's order even then: the frame falls back to it should the pilot not run) */
    e = rt_sched_order(c->sched, c->d_flags, W, hl, pn2, (uint32_t)c->lights.size(), c->max_depth, c->d_order, st);
    if (e) return hip_fail(c, (hipError_t)e, "tile order");
    /* speculated mesh pixels: the silhouettes' neighbours run as long chains (RT_SPLIT_SPEC=2: every
       probe-hit pixel speculated — a test knob that makes repairs happen) */
    const uint32_t spec_row = split && c->split_spec == 1 ? W : 0u;
    /* the probe steps per ray above which a mesh pixel runs as a long chain (none / 200 measured slower,
       profiles/r05ak) */
    const uint32_t long_steps = 96;
    e = rt_sched_box_scan(c->sched, c->d_flags, (uint32_t)npx, pn2, split ? long_steps * pn2 : 0u, spec_row, st);
    if (e) return hip_fail(c, (hipError_t)e, "box-pixel scan");
    uint32_t n_box = 0;
    if (split) { /* every long chain gets a slot: their seed pass and chunks run on a stream of their own */
        HIPCHK(c, hipMemcpyAsync(&n_box, c->sched.scan + npx, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, c->d_split_box.reserve(n_box));
    }
    e = rt_sched_classify(c->sched, (uint32_t)npx, n_box, c->d_class, c->d_split_box, st);
    if (e) return hip_fail(c, (hipError_t)e, "pixel classes");
    c->n_split_box = n_box;
    c->order_key = key;
    c->schedule_rebuilt = true;
    return RT_OK;
}

/* The first frame of a view, whole pixels of many samples: its queue order from a pilot render
   instead of the cost probe.  The probe's few rays per pixel aim their shadow rays at the light
   centres and miss where the samples' rays graze the mesh; the view's next frames are ordered by
   the measured per-pixel costs of the frame before, and the first frame had only
   the probe.  The pilot is the same kernel on the same pixels at pilot_sr^2 samples per pixel,
   with candidate lists built, from a copy of the seeds into a scratch framebuffer and its own
   counters and queue cursors, recording each pixel's traversal steps; the tiles are then sorted
   by them exactly as a measured frame's (rt_sched_order_measured).  Scheduling only: the frame's
   seeds, output and counters are not touched. */
int pilot_order(rt_ctx *c, const RtTriLaunch &a, int trav, int blocks, hipStream_t st)
{
    const size_t seed_words = 2ull * c->wpad * c->hpad, out_floats = (size_t)a.W * a.Hl * 4;
    HIPCHK(c, c->d_pilot_seeds.reserve(seed_words));
    HIPCHK(c, c->d_pilot_out.reserve(out_floats));
    HIPCHK(c, c->d_pilot_cnt.reserve((kCounterBytes + kWorkWords * sizeof(uint32_t)) / sizeof(unsigned long long)));
    HIPCHK(c, hipMemcpyAsync(c->d_pilot_seeds, c->d_seeds, seed_words * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemsetAsync(c->d_pilot_cnt, 0, kCounterBytes + kWorkWords * sizeof(uint32_t), st));
    RtTriLaunch p = a;
    p.seeds = c->d_pilot_seeds;
    p.out = c->d_pilot_out;
    p.progressive = 0;
    p.sample_rate = (uint32_t)c->pilot_sr;
    p.counters = c->d_pilot_cnt;
    p.work_counter = reinterpret_cast<uint32_t *>(c->d_pilot_cnt + RT_COUNTER_WORDS);
    p.take_exact = 0; /* a short-task launch: batched takes from the multi-head queue */
    p.queue_batch = RT_QUEUE_BATCH;
    p.pixel_stats = nullptr;
    p.pixel_iter = c->d_pixel_iter;
    int e = rt_launch_tris(p, trav, false, blocks, st);
    if (!e) e = rt_sched_order_measured(c->sched, c->d_pixel_iter, a.W, a.Hl, 1u, c->d_order, st);
    if (e) return hip_fail(c, (hipError_t)e, "pilot render");
    return RT_OK;
}

/* An owner-map tile's frame stripes, in tile order, on the device (RtTriLaunch::stripe_map);
   re-uploaded (after the stream's earlier renders) only when they change. */
static int upload_stripe_map(rt_ctx *c, uint32_t H, const rt_tile *t, hipStream_t st)
{
    const uint32_t ns = (H + t->stripe_rows - 1) / t->stripe_rows;
    std::vector<uint32_t> mine;
    for (uint32_t s = 0; s < ns; ++s) {
        if (t->stripe_owner[s] >= t->n_ranks) return fail(c, RT_ERR_ARG, "stripe owner out of range");
        if (t->stripe_owner[s] == t->rank) mine.push_back(s);
    }
    if (mine == c->stripe_map_h && c->d_stripe_map) return RT_OK;
    HIPCHK(c, hipStreamSynchronize(st)); /* earlier renders on this stream read the old map */
    if (c->sync_stream && c->sync_stream != st) HIPCHK(c, hipStreamSynchronize(c->sync_stream));
    HIPCHK(c, c->d_stripe_map.reserve(std::max<size_t>(mine.size(), 1)));
    if (!mine.empty())
        HIPCHK(c, hipMemcpy(c->d_stripe_map, mine.data(), mine.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->stripe_map_h = std::move(mine);
    ++c->stripe_map_serial;
    return RT_OK;
}

/* the device's counter words as rt_counters (pixels_long is the caller's) */
rt_counters counters_of(const unsigned long long *h)
{
    rt_counters r{};
    r.rays_closest = h[0];
    r.rays_shadow = h[1];
    r.nodes_visited = h[2];
    r.tris_tested = h[3];
    r.leaves_visited = h[4];
    r.lane_slots = h[5];
    r.clocks_traversal = h[6] / 64; /* summed over every lane of a wave */
    r.clocks_total = h[7] / 64;
    r.rays_skipped = h[RT_CNT_SKIPPED];
    r.clocks_shade = h[RT_CNT_SHADE] / 64;
    r.pixel_clocks_max = h[10];
    r.pixel_rays_max = h[11];
    r.pixel_steps_max = h[12];
    return r;
}

/* ---- rt_render_async, step by step: the order of the steps is the order of the HIP calls on the
   render's stream and of the writes to the context; where it is load-bearing, the step says so.
   One rt_render_async call: its arguments, and what the steps before the launch work out. */
struct Frame {
    float *out;
    uint32_t W, H, prog;
    int kernel;
    const rt_tile *tile;
    int flags;
    hipStream_t st;
    uint32_t hl = 0; /* the tile's rows */
    size_t out_bytes = 0;
    float *dout = nullptr; /* the device framebuffer: the caller's, or the staging area */
    uint32_t stripe = 1, nr = 1, rk = 0, map_key = 0;
    const uint32_t *smap = nullptr;
    bool masked = false; /* under a stop plane (rt_set_tile_stop): whole pixels of its live tiles only */
};

/* The triangle launch's plan. */
struct TriPlan {
    int trav = 0, blocks = 0, blocks_split = 0;
    uint64_t item_blocks = 0, npx = 0, list_cap = 0;
    bool short_frame = false, record_iter = false, lists = false, build_lists = false, pilot = false;
    double sched_ms = 0.0;
};

int render_args(rt_ctx *c, const Frame &f)
{
    const rt_tile *tile = f.tile;
    if (!f.out) return fail(c, RT_ERR_ARG, "null output buffer");
    if (f.kernel < RT_KERNEL_SPHERES || f.kernel > RT_KERNEL_TRIS) return fail(c, RT_ERR_ARG, "unknown kernel");
    if (tile && tile->n_ranks > 1 && (tile->stripe_rows == 0 || tile->rank >= tile->n_ranks))
        return fail(c, RT_ERR_ARG, "bad tile");
    if (tile && tile->n_ranks > 1 && f.kernel == RT_KERNEL_SPHERES && f.prog > 0 && !(f.flags & RT_SEEDS_HALO))
        return fail(c, RT_ERR_ARG,
                    "row-shifted seeds (raytracer.cl:20-30) cross stripe boundaries: progressive sphere frames on "
                    "a tile need the seed-row halo (rt_pack_seed_rows / rt_unpack_seed_rows, flag RT_SEEDS_HALO)");
    if (f.kernel == RT_KERNEL_TRIS && c->n_tris == 0) return fail(c, RT_ERR_NO_MESH, "no mesh set");
    if (f.kernel != RT_KERNEL_TRIS && c->spheres.empty()) return fail(c, RT_ERR_NO_SCENE, "no spheres set");
    if (c->stop_plane) { /* never a silent full render */
        if (f.kernel != RT_KERNEL_TRIS) return fail(c, RT_ERR_ARG, "a tile stop plane is set: it masks raytrace_tris renders only");
        if (tile) return fail(c, RT_ERR_ARG, "a tile stop plane is set: it masks whole frames, not tiles");
        if (f.W != c->stop_w || f.H != c->stop_h) return fail(c, RT_ERR_ARG, "a tile stop plane is set for another frame size");
    }
    return RT_OK;
}

/* RayTracerCL.cpp:229-249: NDRange padding, camera/seed refresh */
int refresh_view(rt_ctx *c, uint32_t W, uint32_t H)
{
    const uint32_t wpad = ((W & 0x1F) == 0) ? W : ((W & 0xFFFFFFE0u) + 0x20u);
    const uint32_t hpad = (uint32_t)std::ceil(H / (float)c->nd_y) * c->nd_y;
    if (W != c->width || H != c->height) {
        c->cam_dirty = false;
        c->width = W;
        c->height = H;
        c->cam = frame_camera(c, W);
        if (c->user_seeds && c->wpad == wpad && c->hpad == hpad) {
            c->user_seeds = false; /* caller-provided seeds for this layout */
        } else {
            const int r = ensure_seeds(c, wpad, hpad, nullptr);
            if (r != RT_OK) return r;
            c->user_seeds = false;
        }
    } else if (c->cam_dirty) {
        c->cam_dirty = false;
        c->cam = frame_camera(c, W);
    }
    if (c->wpad < W || c->hpad < H) return fail(c, RT_ERR_STATE, "seed layout smaller than the frame");
    return RT_OK;
}

/* a rank with no rows: nothing rendered, and nothing of an earlier render reported */
int empty_tile(rt_ctx *c, int kernel)
{
    if (c->sync_stream) HIPCHK(c, hipStreamSynchronize(c->sync_stream)); /* its counter copy has landed */
    memset(c->h_counters, 0, kCounterBytes + sizeof(unsigned long long));
    c->info = rt_render_info{};
    c->info.kernel = (uint32_t)kernel;
    c->info_list_pending = false;
    c->last_long = 0;
    c->sync_stream = nullptr;
    return RT_OK;
}

/* a host framebuffer renders into the staging area (a progressive frame: on top of its upload) */
int stage_output(rt_ctx *c, Frame &f)
{
    f.out_bytes = (size_t)f.W * f.hl * 4 * sizeof(float);
    f.dout = f.out;
    if (!(f.flags & RT_OUT_DEVICE)) {
        HIPCHK(c, c->d_stage.reserve(f.out_bytes / sizeof(float)));
        f.dout = c->d_stage;
        if (f.prog > 0) HIPCHK(c, hipMemcpyAsync(f.dout, f.out, f.out_bytes, hipMemcpyHostToDevice, f.st));
    }
    return RT_OK;
}

int order_streams(rt_ctx *c, Frame &f)
{
    /* a render on another stream than the last one's: ordered after that render's counter hand-back
       (which reads and zeroes the counters and queue cursors this render uses) */
    if (const int r = wait_last_render(c, f.st)) return r;
    if (c->aux_stream) { /* and after a feature / denoise call enqueued since (rt_display.cpp) */
        if (const int r = wait_aux(c, f.st)) return r;
        c->aux_stream = nullptr;
    }
    /* the counters, the guard word and the queue cursors: one memset (none when the last render's
       k_counters_out left them zeroed) */
    if (!c->counters_zeroed)
        HIPCHK(c, hipMemsetAsync(c->d_counters, 0, kCounterBytes + kWorkWords * sizeof(uint32_t), f.st));
    c->counters_zeroed = false;
    const rt_tile *tile = f.tile;
    f.stripe = tile ? tile->stripe_rows : 1u;
    f.nr = tile ? std::max(tile->n_ranks, 1u) : 1u;
    f.rk = tile ? tile->rank : 0u;
    /* an owner-map tile: its stripes' frame indices on the device (the view and schedule keys
       carry the map's serial) */
    if (tile && f.nr > 1 && tile->stripe_owner) {
        const int r = upload_stripe_map(c, f.H, tile, f.st);
        if (r != RT_OK) return r;
        f.smap = c->d_stripe_map;
    }
    f.map_key = f.smap ? c->stripe_map_serial : 0u;
    return RT_OK;
}

/* what the triangle and the sphere launch have in common */
template <class Launch> void common_fields(Launch &a, const rt_ctx *c, const Frame &f)
{
    a.out = f.dout;
    a.seeds = c->d_seeds;
    a.cam = c->cam;
    a.W = f.W;
    a.H = f.H;
    a.Wpad = c->wpad;
    a.Hpad = c->hpad;
    a.Hl = f.hl;
    a.sample_rate = c->sample_rate;
    a.max_depth = c->max_depth;
    a.progressive = f.prog;
    a.stripe = f.stripe;
    a.n_ranks = f.nr;
    a.rank = f.rk;
    a.stripe_map = f.smap;
    a.counters = c->d_counters;
}

/* the mesh, its trees and the lights */
int tri_scene(rt_ctx *c, RtTriLaunch &a)
{
    a.nodes = trav_nodes(c);
    a.shadow_root = trav_kind(c) == RT_TRAV_BVH4Q ? c->shadow_root : 0u; /* the shadow tree: compressed nodes only */
    /* The cone split's subtree A holds every triangle a shadow query aimed at the lights it was made
       for can accept (rt_bvh.cpp never_occludes): the queries start there while every current light
       is, bit for bit, one of those, and the records are the build's.  Any other light (a later
       rt_set_spheres), or a refit since, and they walk the whole shadow tree, which answers for any. */
    bool cone = a.shadow_root && c->cone_root && !c->cone_stale;
    for (size_t l = 0; cone && l < c->lights.size(); ++l) {
        const float w[4] = {c->lights[l].center.x, c->lights[l].center.y, c->lights[l].center.z, c->lights[l].radius};
        bool found = false;
        for (size_t k = 0; !found && k + 4 <= c->cone_lights.size(); k += 4) found = !memcmp(w, &c->cone_lights[k], sizeof(w));
        cone = found;
    }
    if (cone) a.shadow_root = c->cone_root;
    if (trav_kind(c) == RT_TRAV_BVH4Q && c->shadow_cache) {
        /* the cut: a level below the root (A's, when the queries start there), by default
           kShadowCutDepth or, in a shallow tree, the middle level */
        const auto &lv = cone ? c->cone_levels : c->shadow_levels;
        const size_t nl = lv.size();
        const size_t d = c->shadow_cache_depth >= 0 ? (size_t)c->shadow_cache_depth
                                                    : std::min<size_t>(kShadowCutDepth, (nl - (nl > 0)) / 2);
        /* (the lane's word is the node's index in its level, 16 bits: a wider level is no cut) */
        if (d >= 1 && d < nl && lv[d].second - lv[d].first <= 0xffffu) {
            a.shadow_cut_lo = lv[d].first;
            a.shadow_cut_hi = lv[d].second;
        }
    }
    a.tris = c->d_tris;
    a.n_tris = c->n_tris;
    a.lights = c->d_lights;
    a.n_lights = (uint32_t)c->lights.size();
    if (a.n_lights > 16) return fail(c, RT_ERR_LIMIT, "more than 16 emissive spheres");
    return RT_OK;
}

/* the persistent grids, the short-frame rule and the spill area */
int plan_grid(rt_ctx *c, const Frame &f, RtTriLaunch &a, TriPlan &p)
{
    const uint64_t items = (uint64_t)((f.W + 7) / 8) * ((f.hl + 7) / 8) * 64;
    p.item_blocks = (items + RT_BLOCK - 1) / RT_BLOCK;
    /* persistent grids: the plain form's and the sample-split form's own occupancy, the
       plain one at most one block per RT_BLOCK queue items */
    int r = grid_blocks(c, p.trav, c->counting, RT_FORM_PLAIN, &p.blocks);
    if (r != RT_OK) return r;
    p.blocks = std::max(1, (int)std::min<uint64_t>((uint64_t)p.blocks, p.item_blocks));
    /* a short frame — a few samples per resident lane (bunny class at 1 spp: 3.2) — runs on
       3 of the 5 blocks per CU: its time is then its costliest pixels' serial paths, which step
       faster on less crowded SIMDs (bunny class 0.54 -> 0.46 ms at 768 of 1280 blocks; the
       dragon frame at 1024 blocks 96.7 -> 101.2 ms: profiles/r04l, r04m) */
    p.short_frame = (uint64_t)f.W * f.hl * c->sample_rate * c->sample_rate <
                    kShortFrameSamplesPerLane * (uint64_t)p.blocks * RT_BLOCK;
    if (p.short_frame) p.blocks = std::max(1, p.blocks * (int)kShortFrameBlocksPerCU / RT_TRIS_WAVES);
    /* scheduling knobs (read every render; test_stepping_knobs_change_no_bits): a smaller grid, the
       stepping round's exit rule */
    if (const uint32_t gb = env_u32("RTMI_GRID_BLOCKS", 0)) p.blocks = std::min(p.blocks, (int)gb);
    if (p.trav == RT_TRAV_BVH4Q) {
        r = grid_blocks(c, p.trav, c->counting, RT_FORM_SPLIT, &p.blocks_split);
        if (r != RT_OK) return r;
    }
    /* the spill area is indexed by blockIdx: sized for twice the larger grid any kernel of
       this render may run with (a sample-split render runs two streams side by side, each on
       its own part of the area) */
    a.spill_cap = spill_cap(c);
    if (a.spill_cap) {
        const int rs = ensure_spill(c, (size_t)std::max<uint64_t>(std::max(p.blocks, p.blocks_split), p.item_blocks) * 2 *
                                           RT_BLOCK * a.spill_cap);
        if (rs != RT_OK) return rs;
    }
    a.spill = c->d_spill;
    return RT_OK;
}

/* the stepping round's knobs, the inline list resolve and the diagnostics pixel */
void stepping_fields([[maybe_unused]] const Frame &f, RtTriLaunch &a, const TriPlan &p)
{
    a.fetch_k = env_u32("RTMI_FETCH_K", kFetchK);
    a.fetch_frac = env_u32("RTMI_FETCH_FRAC", kFetchFrac);
    /* (short frames keep K 0 by default: bunny class at 1 spp 0.425 -> 0.454 ms with K 2) */
    a.inline_k = p.trav == RT_TRAV_BVH4Q
                     ? std::min<uint32_t>(env_u32("RT_INLINE_LIST", p.short_frame ? 0u : kInlineList), RT_INLINE_MAX)
                     : 0u;
    a.inline_passes = 1u + std::min<uint32_t>(env_u32("RT_INLINE_CHAIN", kInlineChain), 8u);
    a.probe_n = probe_n(a.sample_rate);
    a.diag_pixel = 0xffffffffu;
#if RT_DIAG_ONE_PIXEL
    a.diag_k = 1;
    if (const char *v = getenv("RT_DIAG_PIXEL")) { /* diagnostics build only: "x,y[,k]" */
        unsigned dx = 0, dy = 0, dk = 1;
        const int n = sscanf(v, "%u,%u,%u", &dx, &dy, &dk);
        if (n >= 2) a.diag_pixel = dy * f.W + dx;
        if (n == 3) a.diag_k = dk;
    }
#endif
}

/* sample-split tiles: chunks of about spp / 16 samples; the buffers within RT_SPLIT_MB.  Reads
   n_split_box: after tile_order. */
int plan_split(rt_ctx *c, const Frame &f, RtTriLaunch &a, TriPlan &p)
{
    const uint32_t W = f.W, hl = f.hl;
    a.split_chunks = 0;
    if (f.masked) return RT_OK; /* always whole pixels */
    if (!(a.tile_order && p.trav == RT_TRAV_BVH4Q && split_wanted(c, (uint64_t)W * hl, (uint64_t)p.blocks * RT_BLOCK)))
        return RT_OK;
    /* chunks of about spp / 16 samples; seeds stored every quarter chunk, so that the long
       chains' chunks (run after their seed pass, on a nearly idle chip) are 4x shorter:
       8-way tile 22.6 -> 20.x ms */
    const uint32_t spp = c->sample_rate * c->sample_rate;
    const uint32_t fine = std::max(1u, (spp + 63u) / 64u), csz = fine * std::max(1u, ((spp + c->split_nch - 1u) / c->split_nch) / fine);
    const uint32_t nch = (spp + csz - 1u) / csz, nseed = (spp + fine - 1u) / fine + 1u;
    const size_t npx_s = (size_t)W * hl;
    const size_t seed_bytes = npx_s * nseed * 8u, col_bytes = npx_s * spp * 12u;
    if (seed_bytes + col_bytes > (c->split_mb << 20)) return RT_OK;
    const int rs = ensure_split(c, seed_bytes, col_bytes);
    if (rs != RT_OK) return rs;
    a.split_chunks = nch;
    a.split_chunk = csz;
    a.split_fine = fine;
    a.split_nseed = nseed;
    a.split_seed = c->d_split_seed;
    a.split_col = c->d_split_col;
    a.split_counter = c->d_split_counter;
    a.split_which = c->n_split_box ? RT_SPLIT_MESH : RT_SPLIT_ALL;
    a.split_box = c->d_split_box;
    a.split_n_box = c->n_split_box;
    a.n_nodes4 = c->bvh.n_nodes4;
    /* lanes per long chain: seed_width (a power of two, 8-64) subtree-parallel lanes
       (k_chain_seeds); RT_SEED_COOP4 (3): 4 cooperative lanes (coop_round) where the
       group's LDS stack holds the tree's worst depth-first stack (+ a candidate list's
       blocks); else one */
    const uint32_t sw = c->seed_width ? c->seed_width : seed_width_auto((uint64_t)W * hl, (uint64_t)p.blocks * RT_BLOCK);
    a.split_coop = sw >= 4 ? std::min(64u, std::max(8u, 1u << (31 - __builtin_clz(sw))))
                 : sw == RT_SEED_COOP4 && c->bvh.stack4 + 4 <= RT_COOP_STACK ? RT_SEED_COOP4 : 0u;
    /* a round of 4 nodes adds at most 12 entries and a one-item depth-first walk at
       most the tree's worst stack: rounds take 4 items up to this depth (coop_round) */
    a.coop_multi_sp = std::max(0, (int)RT_COOP_STACK - 12 - (int)c->bvh.stack4);
    if (c->split_spec && a.split_which == RT_SPLIT_MESH) {
        const int rp = spec_setup(c, a, npx_s, f.st);
        if (rp != RT_OK) return rp;
    }
    /* the box pixels' seed pass (one lane per pixel) keeps its blocks resident beside
       the mesh pixels' kernels, whose grids leave room for it */
    const int box_blocks = c->n_split_box ? split_box_blocks(c, std::max(1u, a.split_coop), p.blocks) : 0;
    c->split_box_grid = box_blocks;
    /* the mesh pixels' seed pass: at least one lane per queue item (RT_SEED_GRID_ITEMS), so no lane
       walks two pixels' chains in turn (the blocks beyond residency start as others end) */
    a.split_seed_blocks = (uint32_t)std::max(1, p.blocks - box_blocks);
    if (RT_SEED_GRID_ITEMS) a.split_seed_blocks = (uint32_t)std::max<uint64_t>(a.split_seed_blocks, p.item_blocks);
    p.blocks = std::max(1, std::min((int)std::min<uint64_t>((uint64_t)p.blocks_split, p.item_blocks * nch),
                                    p.blocks_split - box_blocks));
    return RT_OK;
}

/* how the launch takes from its queue, and the off-mesh bounds */
void queue_policy(const rt_ctx *c, RtTriLaunch &a, const TriPlan &p)
{
    /* whole pixels of many samples (long tasks, a few dequeues per microsecond): queue takes of
       exactly the items the idle lanes need, so no wave holds the queue's last tiles back */
    a.take_exact = !a.split_chunks && c->sample_rate * c->sample_rate >= 16u ? 1u : 0u;
    /* short frames: box-path queries whose segment misses the mesh's padded bounds are answered
       without a traversal (bunny class 0.469 -> 0.457 ms; the dragon frame measured 87.1 -> 88.4
       ms with it, profiles/r05ah; the 2-way tile within noise, r05bj: off there) */
    a.mesh_bounds = c->mesh_bounds_ok && p.short_frame ? 1u : 0u;
    for (int k = 0; k < 3; ++k) {
        a.mesh_lo[k] = c->mesh_lo[k];
        a.mesh_hi[k] = c->mesh_hi[k];
    }
    /* short whole-pixel frames take from the multi-head queue (mq_take) in batches of
       RT_QUEUE_BATCH items (0: one head; bunny class 0.519 -> 0.473 ms, profiles/r05ac) */
    a.queue_batch = a.take_exact || a.split_chunks ? 0u : RT_QUEUE_BATCH;
    /* long tasks take exactly from the multi-head queue too: each head's tiles go to the waves
       of one XCD's blocks, so a tile's pixels share that XCD's L2 (dragon frame 87.4 -> 86.5 ms,
       profiles/r05ar) */
    if (a.take_exact) a.queue_batch = 64u;
    /* a split tile's mesh chunk tasks from the heads too, in batches of 64, a tile's chunk layers on
       one head (8-way tile 15.95 -> 15.71 ms, profiles/r05au) */
    if (a.split_chunks) a.queue_batch = 64u;
}

/* a frame under the probe's order records its pixels' costs for the next frame (a sample-split
   frame: its mesh pixels' chunk tasks; the long chains' entries stay 0) */
int record_costs(rt_ctx *c, const Frame &f, RtTriLaunch &a, TriPlan &p)
{
    a.pixel_iter = nullptr;
    /* (frames of >= 16 samples per pixel: a 1-spp pixel's cost is one random path, and the bunny
       class measured 0.436 -> 0.459 ms re-sorted by it, profiles/r05aj) */
    /* (not from a masked frame: its stopped tiles' pixels would record nothing) */
    if (!f.masked && a.tile_order && !c->order_measured && c->sample_rate * c->sample_rate >= 16u) {
        const uint32_t nch = a.split_chunks ? a.split_chunks : 1u;
        const size_t n_i = (size_t)f.W * f.hl * nch;
        HIPCHK(c, c->d_pixel_iter.reserve(2 * n_i));
        if (a.split_chunks) HIPCHK(c, hipMemsetAsync(c->d_pixel_iter, 0, 2 * n_i * sizeof(uint32_t), f.st));
        a.pixel_iter = c->d_pixel_iter;
        c->iter_nch = nch;
        p.record_iter = true;
    }
    return RT_OK;
}

/* diagnostics (RT_DEBUG_LAUNCH): the launch shape */
void debug_launch(const rt_ctx *c, const RtTriLaunch &a, const TriPlan &p)
{
    if (getenv("RT_DEBUG_LAUNCH"))
        fprintf(stderr,
                "[rtmi %p] k_tris trav %d count %d grid %d x %d, spill_cap %u, order %p, split %u x %u, long %u\n",
                (const void *)c, p.trav, (int)c->counting, p.blocks, RT_BLOCK, a.spill_cap, (const void *)a.tile_order,
                a.split_chunks, a.split_chunk, a.split_n_box);
}

/* diagnostics (RT_PIXEL_STATS): per-pixel start/finish clocks (+ queries, steps and the wall clocks
   by phase in a counting launch: 8 x u32 per pixel), dumped raw to $RT_PIXEL_STATS */
int pixel_stats_begin(rt_ctx *c, const Frame &f, RtTriLaunch &a, DevBuf<uint32_t> &stats, const char **path)
{
    *path = getenv("RT_PIXEL_STATS");
    a.pixel_stats = nullptr;
    if (*path) {
        HIPCHK(c, stats.reserve((size_t)f.W * f.hl * 8));
        HIPCHK(c, hipMemsetAsync(stats, 0, (size_t)f.W * f.hl * 32, f.st));
        a.pixel_stats = stats;
    }
    return RT_OK;
}

int pixel_stats_dump(rt_ctx *c, const Frame &f, DevBuf<uint32_t> &stats, const char *path)
{
    if (!stats) return RT_OK;
    std::vector<uint32_t> h((size_t)f.W * f.hl * 8);
    HIPCHK(c, hipMemcpyAsync(h.data(), stats, h.size() * 4, hipMemcpyDeviceToHost, f.st));
    HIPCHK(c, hipStreamSynchronize(f.st));
    stats.reset();
    if (FILE *fp = fopen(path, "wb")) {
        fwrite(h.data(), 4, h.size(), fp);
        fclose(fp);
    }
    return RT_OK;
}

/* diagnostics (RT_LIST_STATS): candidate list lengths */
int list_stats(rt_ctx *c, const Frame &f, const TriPlan &p)
{
    std::vector<uint16_t> h((size_t)p.npx);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->d_list_code, h.size() * 2, hipMemcpyDeviceToHost, f.st));
    HIPCHK(c, hipStreamSynchronize(f.st));
    uint64_t b[7] = {}, sum = 0, nl = 0;
    for (uint16_t code : h) {
        const uint32_t v = code == RT_LIST_NONE ? 255u : code == RT_LIST_EMPTY ? 0u : (code & (RT_LIST_MAX - 1u)) + 1u;
        b[v == 0 ? 0 : v <= 8 ? 1 : v <= 16 ? 2 : v <= 24 ? 3 : v <= 32 ? 4 : v <= 64 ? 5 : 6]++;
        if (v <= RT_LIST_MAX) sum += v, nl++;
    }
    fprintf(stderr, "lists: 0:%llu 1-8:%llu 9-16:%llu 17-24:%llu 25-32:%llu 33-64:%llu none:%llu mean %.2f\n",
            (unsigned long long)b[0], (unsigned long long)b[1], (unsigned long long)b[2],
            (unsigned long long)b[3], (unsigned long long)b[4], (unsigned long long)b[5],
            (unsigned long long)b[6], nl ? (double)sum / (double)nl : 0.0);
    return RT_OK;
}

/* camera-ray candidate lists (k_pixel_lists, rebuilt every frame): a compacted list area
   after the mesh's triangle records in the same buffer (a list block is a leaf code like
   any other), a count and a first slot per pixel.  Leaf codes address slots below 2^28;
   pixels whose list does not fit the area (RT_LIST_MB) take the tree, and a list area
   that cannot be allocated turns the lists off for the render — same bits either way.
   The view key is taken (and stored) before the lists' own key. */
int plan_lists(rt_ctx *c, const Frame &f, RtTriLaunch &a, TriPlan &p)
{
    const uint32_t W = f.W, hl = f.hl;
    const int trav = p.trav;
    a.list_code = nullptr;
    a.list_tile = nullptr;
    const bool bvh4 = c->d_nodes4 && (trav == RT_TRAV_BVH4Q || trav == RT_TRAV_BVH4);
    const uint64_t kept = (c->tree_recs + 7ull) & ~7ull; /* the list area starts on a 128-B line, after the trees' records */
    const uint64_t npx = p.npx = (uint64_t)W * hl;
    uint64_t list_cap = std::min<uint64_t>(npx * RT_LIST_MAX, ((uint64_t)c->list_mb << 20) / 48);
    list_cap = std::min<uint64_t>(list_cap, kept < (1ull << 28) ? (1ull << 28) - 8 - kept : 0);
    /* the view the lists (and the schedule) are a function of */
    const uintptr_t np4 = reinterpret_cast<uintptr_t>(c->d_nodes4.p);
    std::vector<uint32_t> view = {W, f.H, hl, f.stripe, f.nr, f.rk, f.map_key, (uint32_t)trav, (uint32_t)c->mesh_serial,
                                  (uint32_t)(c->mesh_serial >> 32), (uint32_t)np4, (uint32_t)((uint64_t)np4 >> 32)};
    {
        const uint32_t *cb = reinterpret_cast<const uint32_t *>(&c->cam);
        view.insert(view.end(), cb, cb + sizeof(rt_camera) / 4);
    }
    const bool same_view = view == c->last_view;
    c->last_view = view;
    /* The list area: after a build that did not fill its area, a new view's build gets twice
       what the last one took per pixel plus 8 records per pixel (dragon 1080p: 24.9M records
       used of the 89.5M the RT_LIST_MB cap allows), and the buffer gives back the rest; a build
       that filled its area gets the whole cap again (pixels whose list does not fit take the
       tree: the same bits).  The same view keeps the area its lists were built in. */
    bool list_shrink = false;
    if (c->list_cap_last && c->list_used_last < c->list_cap_last && c->list_npx_last) {
        if (same_view) {
            list_cap = std::min<uint64_t>(list_cap, c->list_cap_last);
        } else {
            const uint64_t est = (2 * c->list_used_last * npx + c->list_npx_last - 1) / c->list_npx_last + 8 * npx;
            list_cap = std::min<uint64_t>(list_cap, est);
            list_shrink = true;
        }
    }
    /* Lists pay for their pre-pass (about one traversal per pixel) within one frame from
       sampleRate 4 on; below, from the second frame of a view on, since they are then reused
       (bunny class 1024^2 at 1 spp: a 2.4-ms pre-pass against a 1.0-ms frame) */
    bool lists = (c->pixel_lists == 1 || (c->pixel_lists < 0 && (c->sample_rate >= 4 || same_view))) && bvh4 &&
                 list_cap > 0;
    if (lists && ensure_tris_capacity(c, (size_t)(kept + list_cap), c->tree_recs, f.st, list_shrink) != RT_OK) {
        (void)hipGetLastError(); /* out of device memory: no lists this render */
        lists = false;
    }
    const uint64_t n_tiles = (uint64_t)((W + 7) / 8) * ((hl + 7) / 8);
    if (lists && (c->d_list_code.cap < npx || c->d_list_tile.cap < n_tiles)) {
        c->d_list_code.reset(); /* both again, at this frame's sizes: the lists they held are gone */
        c->d_list_tile.reset();
        c->list_key.clear();
        HIPCHK(c, c->d_list_code.reserve(npx));
        HIPCHK(c, c->d_list_tile.reserve(n_tiles));
    }
    if (lists) HIPCHK(c, c->d_list_alloc.reserve(1));
    if (lists) {
        a.list_code = c->d_list_code;
        a.list_tile = c->d_list_tile;
        a.list_base = (uint32_t)kept;
        a.list_cap = (uint32_t)list_cap;
        a.list_alloc = c->d_list_alloc;
    }
    a.tris = c->d_tris;
    /* The lists depend only on the camera, the mesh and tree, the frame shape and the tile —
       like the BVH and the schedule, they are rebuilt when one of those changes and reused
       by the frames in between (GlutCLWindow refines one view over many frames,
       GlutCLWindow.cpp:151-158; a camera move rebuilds them: bench.py cold_frame_ms). */
    if (lists) {
        const uintptr_t tp = reinterpret_cast<uintptr_t>(c->d_tris.p);
        std::vector<uint32_t> key = view;
        key.insert(key.end(), {(uint32_t)list_cap, (uint32_t)tp, (uint32_t)((uint64_t)tp >> 32)});
        p.build_lists = key != c->list_key;
        c->list_key = key;
    }
    p.lists = lists;
    p.list_cap = list_cap;
    return RT_OK;
}

/* The launches: ev0, the list pre-pass, the pilot, evm, the frame's kernels, ev1.  *e: a launch's
   HIP error, reported by the caller once the render info is filled. */
int launch_tris(rt_ctx *c, const Frame &f, RtTriLaunch &a, TriPlan &p, int *e_out)
{
    hipStream_t st = f.st;
    const int trav = p.trav;
    HIPCHK(c, hipEventRecord(c->ev0, st));
    /* a view's first frame of whole pixels: its order from a pilot render (pilot_order) */
    p.pilot = p.record_iter && !a.split_chunks && c->schedule_rebuilt && c->pilot_sr > 0 && !c->counting &&
              c->sample_rate * c->sample_rate >= kPilotMinSpp;
    int e = p.build_lists ? rt_launch_pixel_lists(a, c->d_nodes4, trav == RT_TRAV_BVH4Q ? c->d_nodes4q.p : nullptr,
                                                  c->d_list_code, c->d_list_tile, st)
                          : 0;
    if (e) c->list_key.clear();
    /* (after the lists: the pilot's camera rays take them, as the frame's do; beside the list
       pre-pass on a second stream, through the tree, it ordered the frame worse: 94.96 against
       98.89 ms, profiles/r06m) */
    if (p.pilot && !e) {
        const int rp = pilot_order(c, a, trav, p.blocks, st);
        if (rp != RT_OK) return rp;
    }
    if (f.masked && !e) {
        /* the queue's order without the stopped tiles, in a buffer of its own (the plane is read here,
           on the render's stream: a borrowed one may have changed since the last render) */
        const uint32_t n_tiles = ((f.W + 7u) / 8u) * ((f.hl + 7u) / 8u);
        rt_ctx::StageTime &t = c->stage_time[RT_ST_STOP_ORDER];
        HIPCHK(c, hipEventRecord(t.e0, st));
        e = rt_launch_order_stop(a.tile_order, c->stop_plane, n_tiles, c->d_stop_order, c->d_stop_order + n_tiles, st);
        HIPCHK(c, hipEventRecord(t.e1, st));
        t.have = true;
        a.tile_order = c->d_stop_order;
    }
    HIPCHK(c, hipEventRecord(c->evm, st));
    if (!e && p.lists && getenv("RT_LIST_STATS"))
        if (const int r = list_stats(c, f, p)) return r;
    /* (only now, the lists built: the default is the whole-pixel launches') */
    if (a.split_chunks && !getenv("RT_INLINE_LIST")) a.inline_k = 0;
    if (!e && a.split_chunks) {
        a.n_recs = (uint32_t)std::min<size_t>(c->tris_cap(), 0xffffffffu); /* the list area included */
        c->last_hit_depth = false;
        e = split_render(c, a, p.blocks, st);
    }
    else if (!e) e = rt_launch_tris(a, trav, c->counting, p.blocks, st);
    if (!e && p.record_iter) c->iter_recorded = true;
    c->last_long = a.split_chunks ? a.split_n_box : 0u;
    HIPCHK(c, hipEventRecord(c->ev1, st));
    *e_out = e;
    return RT_OK;
}

void tris_info(rt_ctx *c, const RtTriLaunch &a, const TriPlan &p)
{
    c->info = rt_render_info{};
    c->info.kernel = RT_KERNEL_TRIS;
    c->info.traversal = (uint32_t)p.trav;
    c->info.grid_blocks = (uint32_t)p.blocks;
    c->info.lists = p.lists ? 1u : 0u;
    c->info.lists_rebuilt = p.build_lists ? 1u : 0u;
    c->info.list_capacity = p.lists ? p.list_cap : 0;
    c->info_list_px = p.lists ? (size_t)p.npx : 0u;
    c->info.pixels_long = c->last_long;
    c->info.split_chunks = a.split_chunks;
    c->info.split_coop = a.split_chunks && a.split_n_box ? a.split_coop : 0u;
    c->info.split_spec = a.split_chunks ? a.split_spec : 0u;
    c->info.split_hit_depth = a.split_chunks && c->last_hit_depth ? 1u : 0u;
    c->info.schedule_measured = a.tile_order && c->order_measured ? 1u : 0u;
    c->info.schedule_rebuilt = c->schedule_rebuilt ? 1u : 0u;
    c->info.schedule_host_ms = p.sched_ms;
    c->info.schedule_pilot = p.pilot ? 1u : 0u;
    c->info.shadow_start = a.shadow_root;
    c->info_list_pending = p.lists;
}

/* The triangle kernel's render.  tile_order runs before the split plan (which reads n_split_box);
   the list pre-pass and the pilot between ev0 and evm. */
int render_tris(rt_ctx *c, const Frame &f, int *e_out)
{
    RtTriLaunch a{};
    TriPlan p;
    common_fields(a, c, f);
    a.map_key = f.map_key;
    a.work_counter = c->d_work;
    if (const int r = tri_scene(c, a)) return r;
    p.trav = trav_kind(c);
    if (const int r = plan_grid(c, f, a, p)) return r;
    stepping_fields(f, a, p);
    a.tile_order = nullptr;
    a.pixel_flags = nullptr;
    a.pixel_class = nullptr;
    const auto h0 = std::chrono::steady_clock::now();
    c->schedule_rebuilt = false;
    if (c->schedule) {
        const int ro = tile_order(c, a, p.blocks, f.st);
        if (ro != RT_OK) return ro;
        a.tile_order = c->d_order;
        a.pixel_flags = a.tile_order ? c->d_flags.p : nullptr;
        a.pixel_class = a.tile_order ? c->d_class.p : nullptr;
    }
    if (const int r = plan_split(c, f, a, p)) return r;
    queue_policy(c, a, p);
    if (const int r = record_costs(c, f, a, p)) return r;
    p.sched_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
    debug_launch(c, a, p);
    DevBuf<uint32_t> stats; /* this render's own: freed at every return */
    const char *stats_path = nullptr;
    if (const int r = pixel_stats_begin(c, f, a, stats, &stats_path)) return r;
    if (const int r = plan_lists(c, f, a, p)) return r;
    if (f.masked) {
        const size_t n_tiles = (size_t)((f.W + 7u) / 8u) * ((f.hl + 7u) / 8u);
        HIPCHK(c, c->d_stop_order.reserve(n_tiles + 1));
        HIPCHK(c, c->stage_time[RT_ST_STOP_ORDER].e0.create());
        HIPCHK(c, c->stage_time[RT_ST_STOP_ORDER].e1.create());
    }
    if (const int r = launch_tris(c, f, a, p, e_out)) return r;
    tris_info(c, a, p);
    return pixel_stats_dump(c, f, stats, stats_path);
}

int render_spheres(rt_ctx *c, const Frame &f, int *e_out)
{
    RtSphLaunch a{};
    common_fields(a, c, f);
    a.spheres = c->d_spheres;
    a.n_spheres = (uint32_t)c->spheres.size();
    HIPCHK(c, hipEventRecord(c->ev0, f.st));
    HIPCHK(c, hipEventRecord(c->evm, f.st));
    *e_out = rt_launch_spheres(a, f.kernel == RT_KERNEL_SPHERES_SS, f.st);
    HIPCHK(c, hipEventRecord(c->ev1, f.st));
    c->info = rt_render_info{};
    c->info.kernel = (uint32_t)f.kernel;
    c->info_list_pending = false;
    return RT_OK;
}

/* the counters (and a new list build's fill) come back on the render's stream, so that
   rt_synchronize is one stream wait (no blocking copy after it); then the frame itself */
int hand_back(rt_ctx *c, const Frame &f)
{
    hipStream_t st = f.st;
    if (c->h_counters_dev && !c->info.lists_rebuilt) {
        /* counters to the host, added to the running totals and zeroed for the next render, in one kernel */
        const int ek = rt_launch_counters_out(c->d_counters, c->h_counters_dev, c->d_totals, (uint32_t)RT_COUNTER_WORDS,
                                              (uint32_t)((kCounterBytes + kWorkWords * sizeof(uint32_t)) / 8u), st);
        if (ek) return hip_fail(c, (hipError_t)ek, "counter hand-back");
        c->counters_zeroed = true;
    } else {
        const int ek = rt_launch_counters_out(c->d_counters, nullptr, c->d_totals, (uint32_t)RT_COUNTER_WORDS, 0u, st);
        if (ek) return hip_fail(c, (hipError_t)ek, "counter totals");
        HIPCHK(c, hipMemcpyAsync(c->h_counters, c->d_counters, kCounterBytes, hipMemcpyDeviceToHost, st));
    }
    if (c->info.lists_rebuilt)
        HIPCHK(c, hipMemcpyAsync(c->h_counters + RT_COUNTER_WORDS, c->d_list_alloc, sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, st));
    if (st != c->stream) HIPCHK(c, hipEventRecord(c->ev_done, st));
    c->sync_stream = st;
    c->have_timing = true;
    c->last_out = f.dout;
    c->last_bytes = f.out_bytes;
    if (!(f.flags & RT_OUT_DEVICE)) HIPCHK(c, hipMemcpyAsync(f.out, f.dout, f.out_bytes, hipMemcpyDeviceToHost, st));
    return RT_OK;
}

} // namespace

extern "C" {

uint32_t rt_tile_rows(uint32_t height, const rt_tile *t)
{
    if (!t || t->n_ranks <= 1) return height;
    if (t->stripe_rows == 0 || t->rank >= t->n_ranks) return 0;
    if (t->stripe_owner) { /* an owner map: the rank's stripes (only the frame's last can be short) */
        uint32_t rows = 0;
        for (uint32_t s = 0, y = 0; y < height; ++s, y += t->stripe_rows)
            if (t->stripe_owner[s] == t->rank) rows += std::min(t->stripe_rows, height - y);
        return rows;
    }
    const uint32_t period = t->stripe_rows * t->n_ranks;
    const uint32_t full = height / period;
    uint32_t rows = full * t->stripe_rows;
    const uint32_t rem = height - full * period;
    const uint32_t start = t->rank * t->stripe_rows;
    if (rem > start) rows += std::min(rem - start, t->stripe_rows);
    return rows;
}

/* A box pixel's serial chain against a mesh pixel of the frame's mean probe steps, in the stripes'
   cost (rt_partition_stripes).  From the 8-way dragon tiles (profiles/r06b/partition8.npz: rank
   time against the rank's long chains and traversal steps, least squares): a long chain adds
   3.5e-4 ms, a whole mesh pixel of the mean steps 6.2e-6 ms — about 55 of them. */
static constexpr uint64_t kPartitionBoxWeight = 55;

int rt_partition_stripes(rt_ctx *c, uint32_t W, uint32_t H, uint32_t stripe, uint32_t n, uint32_t *owner,
                         int *recomputed)
try {
    if (!c || !owner || stripe == 0 || n == 0) return RT_ERR_ARG;
    if (recomputed) *recomputed = 0;
    const uint32_t ns = (H + stripe - 1) / stripe;
    if (ns == 0) return RT_OK;
    const int trav = trav_kind(c);
    if (c->n_tris == 0 || trav != RT_TRAV_BVH4Q || n == 1) { /* nothing to probe (or one rank): interleaved */
        for (uint32_t s = 0; s < ns; ++s) owner[s] = s % n;
        return RT_OK;
    }
    const rt_camera cam = frame_camera(c, W);
    std::vector<uint32_t> key = {W, H, stripe, n, (uint32_t)c->mesh_serial, (uint32_t)(c->mesh_serial >> 32),
                                 (uint32_t)c->lights.size()};
    {
        const uint32_t *cb = reinterpret_cast<const uint32_t *>(&cam);
        key.insert(key.end(), cb, cb + sizeof(rt_camera) / 4);
        for (const rt_sphere &L : c->lights) {
            const uint32_t *lb = reinterpret_cast<const uint32_t *>(&L);
            key.insert(key.end(), lb, lb + sizeof(rt_sphere) / 4);
        }
    }
    if (key == c->part_key && c->part_owner.size() == ns) {
        std::copy(c->part_owner.begin(), c->part_owner.end(), owner);
        return RT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (const int r = wait_last_render(c, st)) return r;
    if (const int r = wait_aux(c, st)) return r;
    const size_t npx = (size_t)W * H;
    if (c->d_part_probe.cap < npx) { /* (an earlier probe on the stream may still use the old area) */
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, c->d_part_probe.reserve(npx));
    }
    if (c->d_part_cost.cap < (size_t)ns * 2) {
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, c->d_part_cost.reserve((size_t)ns * 2));
    }
    /* the probe of the whole frame: one camera ray per pixel (its centre) and its shadow rays */
    RtTriLaunch a{};
    a.nodes = trav_nodes(c);
    a.tris = c->d_tris;
    a.n_tris = c->n_tris;
    a.lights = c->d_lights;
    a.n_lights = (uint32_t)c->lights.size();
    a.cam = cam;
    a.W = W;
    a.H = H;
    a.Hl = H;
    a.stripe = 1;
    a.n_ranks = 1;
    a.rank = 0;
    a.stripe_map = nullptr;
    a.probe_n = 1;
    int blocks = 0;
    if (const int r = grid_blocks(c, trav, false, RT_FORM_PLAIN, &blocks)) return r;
    a.spill_cap = spill_cap(c);
    if (a.spill_cap) {
        HIPCHK(c, hipStreamSynchronize(st)); /* (a render in flight may use the spill area) */
        if (const int r = ensure_spill(c, (size_t)blocks * 2 * RT_BLOCK * a.spill_cap)) return r;
    }
    a.spill = c->d_spill;
    int e = rt_launch_probe_cost(a, blocks, c->d_part_probe, st);
    if (!e) e = rt_launch_stripe_costs(c->d_part_probe, W, H, stripe, 1u, c->d_part_cost, st);
    if (e) return hip_fail(c, (hipError_t)e, "partition probe");
    std::vector<unsigned long long> h((size_t)ns * 2);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->d_part_cost, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    /* a stripe's cost in probe steps: its mesh pixels' steps + its box pixels at kPartitionBoxWeight
       mesh pixels of the frame's mean steps each (integers: every rank gets the same map) */
    uint64_t mesh_px = 0, mesh_steps = 0;
    for (uint32_t s = 0; s < ns; ++s) {
        const uint64_t px = (uint64_t)W * std::min(stripe, H - s * stripe);
        mesh_px += px - h[2 * s];
        mesh_steps += h[2 * s + 1];
    }
    const uint64_t box_cost = kPartitionBoxWeight * (mesh_px ? (mesh_steps + mesh_px / 2) / mesh_px : 1u);
    std::vector<uint64_t> cost(ns);
    for (uint32_t s = 0; s < ns; ++s) cost[s] = h[2 * s] * box_cost + h[2 * s + 1] + 1u;
    /* LPT: costliest stripe first (ties: lower index), to the least loaded rank (ties: lower rank) */
    std::vector<uint32_t> order(ns);
    for (uint32_t s = 0; s < ns; ++s) order[s] = s;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cost[x] > cost[y]; });
    std::vector<uint64_t> load(n, 0);
    for (uint32_t s : order) {
        uint32_t best = 0;
        for (uint32_t r = 1; r < n; ++r)
            if (load[r] < load[best]) best = r;
        owner[s] = best;
        load[best] += cost[s];
    }
    c->part_key = key;
    c->part_owner.assign(owner, owner + ns);
    if (recomputed) *recomputed = 1;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_render_async(rt_ctx *c, float *out, uint32_t W, uint32_t H, uint32_t prog, int kernel, const rt_tile *tile,
                    int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (W == 0 || H == 0) return RT_OK; /* RayTracerCL.cpp:219-220 */
    Frame f = {out, W, H, prog, kernel, tile, flags, nullptr};
    if (const int r = render_args(c, f)) return r;
    f.masked = c->stop_plane != nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    f.st = stream ? (hipStream_t)stream : c->stream;
    if (const int r = refresh_view(c, W, H)) return r;
    f.hl = rt_tile_rows(H, tile);
    if (f.hl == 0) return empty_tile(c, kernel);
    if (const int r = stage_output(c, f)) return r;
    if (const int r = order_streams(c, f)) return r;
    int e = 0;
    if (const int r = kernel == RT_KERNEL_TRIS ? render_tris(c, f, &e) : render_spheres(c, f, &e)) return r;
    if (e) return hip_fail(c, (hipError_t)e, "kernel launch");
    return hand_back(c, f);
} RT_CATCH(err_of(c))

int rt_set_tile_stop(rt_ctx *c, const uint32_t *stop, uint32_t W, uint32_t H, int flags)
try {
    if (!c) return RT_ERR_ARG;
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_set_tile_stop: flags other than RT_OUT_DEVICE");
    if (!stop) { /* cleared: the renders are whole frames again */
        c->stop_plane = nullptr;
        c->stop_w = c->stop_h = 0;
        return RT_OK;
    }
    if (!W || !H || (uint64_t)W * H >= (1ull << 28)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & RT_OUT_DEVICE) {
        c->stop_plane = stop; /* borrowed: read on each render's stream */
    } else {
        HIPCHK(c, hipSetDevice(c->device));
        /* a render in flight may still read the last copy */
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->sync_stream && c->sync_stream != c->stream) HIPCHK(c, hipStreamSynchronize(c->sync_stream));
        const size_t n_tiles = (size_t)((W + 7u) / 8u) * ((H + 7u) / 8u);
        c->stop_plane = nullptr;
        HIPCHK(c, c->d_stop_own.reserve(n_tiles));
        HIPCHK(c, hipMemcpy(c->d_stop_own, stop, n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice));
        c->stop_plane = c->d_stop_own;
    }
    c->stop_w = W;
    c->stop_h = H;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_synchronize(rt_ctx *c)
try {
    if (!c) return RT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->sync_stream && c->sync_stream != c->stream) HIPCHK(c, hipStreamSynchronize(c->sync_stream));
    if (c->aux_stream) HIPCHK(c, hipEventSynchronize(c->ev_aux));
    const unsigned long long *h = c->h_counters;
    if (c->info.lists_rebuilt) { /* the list area the new lists took: sizes the next build's area */
        const uint32_t used = (uint32_t)(h[RT_COUNTER_WORDS] & 0xffffffffu);
        c->list_used_last = used;
        c->list_cap_last = c->info.list_capacity;
        c->list_npx_last = c->info_list_px;
    }
    c->last = counters_of(h);
    c->last.pixels_long = c->last_long;
    c->info.split_repaired = (uint32_t)h[RT_CNT_REPAIR];
    if (h[RT_CNT_GUARD]) { /* a defect guard of the long chains' seed pass: the frame is not the reference's */
        c->info.split_guard = (uint32_t)h[RT_CNT_GUARD];
        char msg[160];
        snprintf(msg, sizeof(msg),
                 "sample-split seed pass: a defect guard fired (flags 0x%x: 1 record index, 2 group stack, 4 round "
                 "bound); the frame is invalid (RT_SPLIT=0 renders whole pixels)",
                 (unsigned)h[RT_CNT_GUARD]);
        return fail(c, RT_ERR_STATE, msg);
    }
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_counter_totals(rt_ctx *c, rt_counters *sum, uint64_t *renders, int reset)
try {
    if (!c || !sum) return RT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->sync_stream && c->sync_stream != c->stream) HIPCHK(c, hipStreamSynchronize(c->sync_stream));
    unsigned long long h[RT_COUNTER_WORDS + 1];
    HIPCHK(c, hipMemcpy(h, c->d_totals, sizeof(h), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(c, hipMemset(c->d_totals, 0, sizeof(h)));
    *sum = counters_of(h);
    if (renders) *renders = h[RT_COUNTER_WORDS];
    if (h[RT_CNT_GUARD]) {
        char msg[160];
        snprintf(msg, sizeof(msg),
                 "rt_counter_totals: a sample-split seed pass defect guard fired in one of the renders (flags 0x%x); "
                 "those frames are invalid",
                 (unsigned)h[RT_CNT_GUARD]);
        return fail(c, RT_ERR_STATE, msg);
    }
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_render(rt_ctx *c, float *out, uint32_t W, uint32_t H, uint32_t prog, int kernel, const rt_tile *tile,
              int flags)
try {
    const int r = rt_render_async(c, out, W, H, prog, kernel, tile, flags, nullptr);
    if (r != RT_OK) return r;
    return rt_synchronize(c); /* cmdQueue.finish(), RayTracerCL.cpp:292 */
} RT_CATCH(err_of(c))

static int seed_rows_io(rt_ctx *c, const uint32_t *rows, uint32_t n, uint32_t *buf, int flags, bool unpack)
{
    if (!c || (n && (!rows || !buf))) return RT_ERR_ARG;
    if (!c->wpad) return fail(c, RT_ERR_STATE, "no seed layout");
    for (uint32_t i = 0; i < n; ++i)
        if (rows[i] >= c->hpad) return fail(c, RT_ERR_ARG, "seed row out of range");
    if (!n) return RT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t words = 2ull * n * c->wpad;
    HIPCHK(c, c->d_halo_rows.reserve(n));
    uint32_t *dbuf = buf;
    const bool on_device = (flags & RT_OUT_DEVICE) != 0;
    if (!on_device) {
        HIPCHK(c, c->d_halo_buf.reserve(words));
        dbuf = c->d_halo_buf;
        if (unpack) HIPCHK(c, hipMemcpyAsync(dbuf, buf, words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->d_halo_rows, rows, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const int e = rt_launch_seed_rows(c->d_seeds, c->wpad, c->hpad, c->d_halo_rows, n, dbuf, unpack, c->stream);
    if (e) return hip_fail(c, (hipError_t)e, "seed-row kernel");
    if (!on_device && !unpack)
        HIPCHK(c, hipMemcpyAsync(buf, dbuf, words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_pack_seed_rows(rt_ctx *c, const uint32_t *rows, uint32_t n, uint32_t *buf, int flags)
try {
    return seed_rows_io(c, rows, n, buf, flags, false);
} RT_CATCH(err_of(c))

int rt_unpack_seed_rows(rt_ctx *c, const uint32_t *rows, uint32_t n, const uint32_t *buf, int flags)
try {
    return seed_rows_io(c, rows, n, const_cast<uint32_t *>(buf), flags, true);
} RT_CATCH(err_of(c))

int rt_read(rt_ctx *c, float *host, size_t n_floats)
try {
    if (!c || !host) return RT_ERR_ARG;
    if (!c->last_out) return fail(c, RT_ERR_STATE, "rt_read before any render");
    if (n_floats * sizeof(float) < c->last_bytes) return fail(c, RT_ERR_ARG, "rt_read: host buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(host, c->last_out, c->last_bytes, hipMemcpyDeviceToHost));
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_last_render_info(rt_ctx *c, rt_render_info *out)
try {
    if (!c || !out) return RT_ERR_ARG;
    if (c->info_list_pending) { /* how much of the list area the render's lists took */
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        uint32_t used = 0;
        HIPCHK(c, hipMemcpy(&used, c->d_list_alloc, sizeof(used), hipMemcpyDeviceToHost));
        c->info.list_records = std::min<uint64_t>(used, c->info.list_capacity);
        const size_t npx = c->info_list_px;
        std::vector<uint16_t> h(npx);
        if (npx) HIPCHK(c, hipMemcpy(h.data(), c->d_list_code, npx * 2, hipMemcpyDeviceToHost));
        uint32_t tree = 0;
        for (uint16_t v : h) tree += v == RT_LIST_NONE ? 1u : 0u;
        c->info.list_pixels_tree = tree;
        c->info_list_pending = false;
    }
    *out = c->info;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_last_long_chains(rt_ctx *c, uint32_t *out, uint32_t cap, uint32_t *n)
try {
    if (!c || !n || (cap && !out)) return RT_ERR_ARG;
    *n = c->last_long;
    const uint32_t k = std::min(cap, c->last_long);
    if (!k) return RT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_split_box, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_last_list_counts(rt_ctx *c, uint16_t *out, uint32_t cap, uint32_t *n)
try {
    if (!c || !n || (cap && !out)) return RT_ERR_ARG;
    *n = c->info.lists ? (uint32_t)c->info_list_px : 0u;
    const uint32_t k = std::min(cap, *n);
    if (!k) return RT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_list_code, (size_t)k * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < k; ++i)
        out[i] = out[i] == RT_LIST_NONE ? (uint16_t)0xffffu
                 : out[i] == RT_LIST_EMPTY ? (uint16_t)0u
                                           : (uint16_t)((out[i] & (RT_LIST_MAX - 1u)) + 1u);
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_get_counters(const rt_ctx *c, rt_counters *out)
try {
    if (!c || !out) return RT_ERR_ARG;
    *out = c->last;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_set_counting(rt_ctx *c, int enable)
try {
    if (!c) return RT_ERR_ARG;
    c->counting = enable != 0;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_last_kernel_split_ms(const rt_ctx *c, float *prepass_ms, float *main_ms)
try {
    if (!c || !prepass_ms || !main_ms) return RT_ERR_ARG;
    if (!c->have_timing) return RT_ERR_STATE;
    if (hipEventSynchronize(c->ev1) != hipSuccess) return RT_ERR_HIP;
    if (hipEventElapsedTime(prepass_ms, c->ev0, c->evm) != hipSuccess) return RT_ERR_HIP;
    return hipEventElapsedTime(main_ms, c->evm, c->ev1) == hipSuccess ? RT_OK : RT_ERR_HIP;
} RT_CATCH(err_of(c))

int rt_last_kernel_ms(const rt_ctx *c, float *ms)
try {
    if (!c || !ms) return RT_ERR_ARG;
    if (!c->have_timing) return RT_ERR_STATE;
    if (hipEventSynchronize(c->ev1) != hipSuccess) return RT_ERR_HIP;
    return hipEventElapsedTime(ms, c->ev0, c->ev1) == hipSuccess ? RT_OK : RT_ERR_HIP;
} RT_CATCH(err_of(c))

int rt_trace_rays(rt_ctx *c, const rt_ray *rays, uint32_t n, int any_hit, int32_t *out_idx, float *out_t)
try {
    if (!c || !rays || !out_idx) return RT_ERR_ARG;
    if (!c->n_tris) return fail(c, RT_ERR_NO_MESH, "no mesh set");
    if (n == 0) return RT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<rt_ray> d_rays; /* this call's own: freed at every return */
    DevBuf<int32_t> d_idx;
    DevBuf<float> d_t;
    hipError_t e = d_rays.reserve(n);
    if (e == hipSuccess) e = d_idx.reserve(n);
    if (e == hipSuccess) e = d_t.reserve(n);
    if (e == hipSuccess) e = hipMemcpy(d_rays, rays, n * sizeof(rt_ray), hipMemcpyHostToDevice);
    const uint32_t cap = spill_cap(c);
    if (e == hipSuccess && cap) {
        const int rs = ensure_spill(c, (size_t)n * cap);
        if (rs != RT_OK) return rs;
    }
    if (e == hipSuccess) e = hipEventRecord(c->ev0, c->stream);
    if (e == hipSuccess) e = hipEventRecord(c->evm, c->stream);
    if (e == hipSuccess) {
        /* The tree leaves out triangles no UNIT-length ray can hit (rt_bvh.cpp never_hit); the
           kernels only trace unit directions, but a caller's rays may be longer: then the
           linear loop over every triangle answers (same semantics, all triangles). */
        int kind = trav_kind(c);
        if (c->bvh.n_hit < c->n_tris)
            for (uint32_t i = 0; i < n; ++i) {
                const rt_vec3 &d = rays[i].d;
                if (!((double)d.x * d.x + (double)d.y * d.y + (double)d.z * d.z <= 1.002)) { /* |d| <= 1.001 */
                    kind = RT_TRAV_LINEAR;
                    break;
                }
            }
        c->counters_zeroed = false; /* this trace leaves its counts there */
        if (c->sync_stream && c->sync_stream != c->stream) {
            e = hipStreamWaitEvent(c->stream, c->ev_done, 0); /* (recorded on the caller's stream) */
        }
        if (e == hipSuccess && c->aux_stream && c->aux_stream != c->stream) e = hipStreamWaitEvent(c->stream, c->ev_aux, 0);
        if (e == hipSuccess && c->counting) e = hipMemsetAsync(c->d_counters, 0, RT_COUNTER_WORDS * sizeof(unsigned long long), c->stream);
        if (e == hipSuccess) {
            const int le = rt_launch_trace_rays(trav_nodes(c), c->d_tris, c->n_tris, d_rays, n, any_hit, kind, c->d_spill,
                                                cap, d_idx, d_t, c->counting ? c->d_counters : nullptr, c->stream);
            e = (hipError_t)le;
        }
    }
    if (e == hipSuccess) e = hipEventRecord(c->ev1, c->stream);
    if (e == hipSuccess) c->have_timing = true;
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out_idx, d_idx, n * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_t) e = hipMemcpy(out_t, d_t, n * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && c->counting) { /* rt_get_counters: queries and records of these rays */
        unsigned long long h[RT_N_COUNTERS];
        e = hipMemcpy(h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost);
        c->last = rt_counters{};
        c->last.rays_closest = h[0];
        c->last.rays_shadow = h[1];
        c->last.nodes_visited = h[2];
        c->last.tris_tested = h[3];
        c->last.leaves_visited = h[4];
    }
    if (e != hipSuccess) return hip_fail(c, e, "rt_trace_rays");
    return RT_OK;
} RT_CATCH(err_of(c))

} /* extern "C" */
