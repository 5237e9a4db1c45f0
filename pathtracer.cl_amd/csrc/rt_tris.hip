/*
 * rt_tris.hip — the triangle megakernel of the MI355X path tracer and its launch.
 *
 *   k_tris<TRAV, COUNT, SPLIT, MQ, INL>   raytrace_tris (clrt/ocl/raytracer.cl:184-243), 20 instantiations
 *   tris_kernel                           the one map from a launch's (trav, count, split, mq, inl) to them
 *   rt_launch_tris, rt_tris_grid_blocks   the launch, and the persistent grid's size from its occupancy
 *   k_counters_out, rt_launch_counters_out   a render's counters to the host, zeroed for the next
 *
 * k_tris is a persistent wavefront state machine: every loop iteration each
 * live lane performs exactly ONE ray query (a path segment's closest hit or one
 * shadow ray) through a shared traversal loop, then advances its path.  Lanes
 * whose pixel finished are refilled from a global pixel queue with one
 * ballot + popcount + atomicAdd per wave (prefix-rank assignment), so SIMD
 * lanes stay busy until the queue drains.  The traversal stack lives in LDS
 * ([depth][lane] stride 256: conflict-free), BVH nodes and triangles are
 * 16-B-aligned float4 records read with dwordx4 loads.  See DESIGN.md.
 * The per-lane ray queries themselves (triangle test, stack, traversal steps) are in
 * rt_traverse.h, shared with rt_features.hip; the queue takes, the counters and the camera ray
 * in rt_kernel_util.h, shared with the sample-split seed passes (rt_split.hip).
 */
#include <hip/hip_runtime.h>

#include <array>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "rt_device.h"
#include "rt_internal.h"
#include "rt_quant.h"
#include "rt_traverse.h"
#include "rt_kernel_util.h"

#pragma clang fp contract(off)

namespace {

/* Does the segment o + t d, tmin <= t <= tmax, miss the box [lo, hi]?  Slab test with the hardware
   reciprocal; the box is the mesh's bounds padded far beyond the test's rounding (mesh_bounds), so
   a segment reported missing meets no triangle.  A zero direction component on a slab plane gives
   0 x inf = NaN, which min/max drop (a ray in that plane lies outside the triangles' padded box
   anyway). */
__device__ __forceinline__ bool segment_misses_box(V3 o, V3 d, float tmin, float tmax, const float *lo, const float *hi)
{
    const float ix = __builtin_amdgcn_rcpf(d.x), iy = __builtin_amdgcn_rcpf(d.y), iz = __builtin_amdgcn_rcpf(d.z);
    const float x1 = (lo[0] - o.x) * ix, x2 = (hi[0] - o.x) * ix;
    const float y1 = (lo[1] - o.y) * iy, y2 = (hi[1] - o.y) * iy;
    const float z1 = (lo[2] - o.z) * iz, z2 = (hi[2] - o.z) * iz;
    const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(x1, x2), __builtin_fminf(y1, y2)),
                                     __builtin_fmaxf(__builtin_fminf(z1, z2), tmin));
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(x1, x2), __builtin_fmaxf(y1, y2)),
                                     __builtin_fminf(__builtin_fmaxf(z1, z2), tmax));
    return tn > tf;
}

/* A traversal step's counts (trav_step's TravCounts) in a lane's counters and in its pixel's
   measured cost: the records visited in a counting launch, the trav_step calls otherwise
   (pixel_iter) */
template <bool COUNT>
__device__ __forceinline__ void count_step(unsigned long long (&cnt)[RT_N_COUNTERS], unsigned long long &pix_steps,
                                           const TravCounts &tc)
{
    if (COUNT) {
        cnt[2] += tc.nodes;
        cnt[3] += tc.tests;
        cnt[4] += tc.leaves;
        pix_steps += tc.nodes + tc.leaves;
    } else {
        ++pix_steps;
    }
}

/* ======================================================================== */
/* Triangle kernel: raytrace_tris + trace_path_tri (rtcommon.h:371-470).     */

constexpr int kMaxLights = 16;

enum : int { M_IDLE = 0, M_NEWSAMPLE = 1, M_CLOSEST = 2, M_SHADOW = 3, M_DONE = 4 };

/* Per-lane loop, one iteration:
     D  lanes whose ray query completed advance their path (trace_path_tri) and
        issue the next query, start the next sample, or write the pixel;
     A  idle lanes take the next pixels from the queue;
     B  camera ray of a new sample;
     C  ray queries.  BVH kinds: queries are resumable — newly issued queries
        start, then the wave steps every running query one node (or leaf) at a
        time until `fetch_k` lanes have completed (or none is running), so lanes
        whose query ended early go back to work instead of idling until the
        wave's longest query ends.  LINEAR: each query runs to completion inside
        the iteration (the reference loop, wave-uniform).
   SPLIT: a queue item is one chunk of a pixel's samples, started from the seed the seed pass
   (k_split_seeds) stored for it; each sample's radiance is stored for k_split_finish. */
/* path-advance passes that may answer an off-mesh box-path query in place (0 / 1 / all: bunny class
   0.484 / 0.457 / 0.594 ms, profiles/r05ag-r05ah); later ones at the stepping round's start, without a step */
constexpr int kOffMeshRedo = 1;
/* INL: the instantiations with the inline list resolve of phase B (BVH4Q launches with inline_k > 0);
   the others compile to the loop without it, register for register (the kernel has none to spare) */
template <int TRAV, bool COUNT, bool SPLIT = false, bool MQ = false, bool INL = false> /* MQ: the multi-head queue (mq_take) */
__global__ __launch_bounds__(RT_BLOCK, RT_TRIS_WAVES) void k_tris(RtTriLaunch a)
{
    constexpr bool RESUME = TRAV == RT_TRAV_BVH4 || TRAV == RT_TRAV_BVH4Q;
    __shared__ int s_stack[RT_STACK_DEPTH * RT_BLOCK];
    __shared__ float s_light[kMaxLights * 8];
    /* the pixel sum and the path throughput, touched once per sample / segment, live in LDS
       (6 floats per lane) instead of six registers across the stepping loop */
    __shared__ float s_state[6 * RT_BLOCK];
    /* the lane's pixel's candidate list (list_pack), read when it takes the pixel instead of before
       every camera ray (LDS budget: 5 blocks per CU beside the RT_STACK_DEPTH = 20-entry stack and
       the hit normal: 31,232 B per block, 31,744 B with the shadow cache's words below) */
    __shared__ uint32_t s_list[RT_BLOCK];
    /* the closest hit's unnormalised normal, formed at its accept from the record in registers
       (trav_step_q), so the path advance needs no second fetch of the hit's edges */
    __shared__ float s_hn[3 * RT_BLOCK];
    lds_float *const st_hn = (lds_float *)(s_hn + threadIdx.x);
    /* the shadow cache (rt_traverse.h ShadowCut): the cut node this pixel's last occluded shadow query
       from a mesh hit went through (0: none); 512 B, which the 5 blocks per CU still hold */
    __shared__ uint16_t s_entry[RT_NO_SHADOW_CACHE ? 1 : RT_BLOCK];
    lds_u16 *const st_entry = (lds_u16 *)(s_entry + (RT_NO_SHADOW_CACHE ? 0 : threadIdx.x));
    if (!RT_NO_SHADOW_CACHE) *st_entry = 0;
    float *const st_acc = s_state + threadIdx.x, *const st_prop = s_state + 3 * RT_BLOCK + threadIdx.x;
#define ACC_GET(k) st_acc[(k) * RT_BLOCK]
#define ACC_SET(k, v) (st_acc[(k) * RT_BLOCK] = (v))
#define PROP_GET(k) st_prop[(k) * RT_BLOCK]
#define PROP_SET(k, v) (st_prop[(k) * RT_BLOCK] = (v))

    /* emissive spheres: center.xyz, radius, emission.xyz (materials.h:232, rtcommon.h:97-99) */
    const uint32_t n_lights = a.n_lights < (uint32_t)kMaxLights ? a.n_lights : (uint32_t)kMaxLights;
    if (threadIdx.x < n_lights) {
        const rt_sphere &L = a.lights[threadIdx.x];
        float *dst = s_light + threadIdx.x * 8;
        dst[0] = L.center.x;
        dst[1] = L.center.y;
        dst[2] = L.center.z;
        dst[3] = L.radius;
        dst[4] = L.mat.emission.x;
        dst[5] = L.mat.emission.y;
        dst[6] = L.mat.emission.z;
        dst[7] = 0.0f;
    }
    __syncthreads();

    Stack stk;
    stk.init(s_stack, a.spill, a.spill_cap);
    const float4 *__restrict__ nodes = reinterpret_cast<const float4 *>(a.nodes);
    const float4 *__restrict__ tris = reinterpret_cast<const float4 *>(a.tris);
    float4 *__restrict__ out = reinterpret_cast<float4 *>(a.out);
    const uint32_t spp = a.sample_rate * a.sample_rate;
    const uint32_t tiles_x = (a.W + 7u) >> 3;
    const uint32_t tiles_y = (a.Hl + 7u) >> 3;
    const uint32_t n_items = tiles_x * tiles_y * 64u;
    const uint32_t n_tasks =
        SPLIT ? (a.split_which == RT_SPLIT_BOX ? box_items(a) : n_items) * a.split_chunks
              : n_items;
    /* launch-uniform values pinned to SGPRs (readfirstlane), so they neither occupy nor
       spill vector registers */
    const float hw = uniform_f(((float)a.W) / 2.0f);
    const float hh = uniform_f(((float)a.H) / 2.0f);
    const float mix_t = uniform_f(a.progressive > 0 ? 1.0f / (float)a.progressive : 0.0f);
    const float bw = (float)RT_BOX_WIDTH, bh = (float)RT_BOX_HEIGHT;
    const int fetch_k_all = (int)a.fetch_k;
    const uint32_t inline_k = !INL ? 0u : a.inline_k < (uint32_t)RT_INLINE_MAX ? a.inline_k : (uint32_t)RT_INLINE_MAX;
    const int inline_passes = INL ? (int)a.inline_passes : 0;

    int mode = M_IDLE;
    uint32_t x = 0, yl = 0; /* pixel column and local row (global row / seed slot derived) */
    Seed seed = {0u, 0u};
    float col_x = 0.0f, col_y = 0.0f, col_z = 0.0f; /* this path's radiance (trace_path_tri's pixelColor) */
    uint32_t sample = 0, depth = 0, light = 0;
    /* the query ray: a path segment (closest hit) or a shadow ray from the offset hit
       point (any hit) — one register set for both, the phases never overlap */
    V3 qo = v3(0.0f, 0.0f, 0.0f), qd = v3(0.0f, 0.0f, 1.0f);
    V3 hp = qo, hn = qo, direct = qo;
    float stmax = 0.0f;
    bool tri_hit = false;
    bool running = false; /* a resumable query is in flight */
    /* the pixel's class from the probe: -1 mesh pixel; a box pixel (long sample chain): -2, or
       its slot >= 0 among the long chains of a sample-split render */
    int pclass = -1;
    /* SPLIT over long chains with split_hit_depth: the depth of the sample's mesh hit (the closest
       queries above it meet only the box); 0 otherwise */
    int hit_depth = 0;
    bool fin = false;     /* the lane's query completed: ts.best / ts.best_t hold its result */
    const ShadowCut sc_cut = {a.shadow_cut_lo, RT_NO_SHADOW_CACHE ? 0u : a.shadow_cut_hi - a.shadow_cut_lo,
                              (int)a.shadow_root};
    TravState ts = trav_idle();
    unsigned long long cnt[RT_N_COUNTERS] = {};
    const unsigned long long t_k0 = COUNT ? wave_clock() : 0ull;
    /* counting launches: this pixel's start clock, queries and traversal steps */
    unsigned long long pix_t0 = 0, pix_q = 0, pix_steps = 0;
    /* counting launches with RT_PIXEL_STATS: this pixel's wall clocks by phase (path advance D,
       refill + camera ray A/B, stepping rounds C) and its loop iterations */
    unsigned long long pix_d = 0, pix_ab = 0, pix_c = 0, pix_it = 0;
    uint32_t pix_rt0 = 0; /* pixel start (s_memrealtime), RT_PIXEL_STATS diagnostics */
    uint32_t bnext = 0, bend = 0; /* the wave's batch of queue items (batch_take) */
    /* the multi-head queue (mq_take: launches of 64-item groups with batched takes) */
    const bool multi_q = MQ; /* multi-head queue: short frames' batched takes, long tasks' exact takes (batch 0)
                                and a split tile's mesh chunk tasks; never for RT_SPLIT_BOX launches */
    uint32_t qs = (blockIdx.x % RT_QHEADS) << 4;

    for (;;) {
        /* INL: D, A and B run again (one copy of each, a jump back from the end of B) when B resolved
           camera rays against their candidate lists (below), so those lanes shade and issue their
           shadow rays before the next stepping round; round 0 is for the lanes the stepping loop
           finished, the idle lanes and the new samples */
        int pass = 0;
    advance:
        const unsigned long long t_d0 = (COUNT || RT_PLAIN_PIXEL_STATS) ? wave_clock() : 0ull;
        /* ---- D: advance the path (trace_path_tri, rtcommon.h:378-468) ---- */
        for (int redo_pass = 0;; ++redo_pass) {
            if (fin) {
                fin = false;
                bool want_shadow = false, seg_done = false, sample_done = false;
                if (mode == M_CLOSEST) {
                    ++cnt[0];
                    if (COUNT || RT_PLAIN_PIXEL_STATS) ++pix_q;
                    bool surface = true;
                    if (ts.best >= 0) {
                        const float qt = ts.best_t;
                        hp = v3(qo.x + qd.x * qt, qo.y + qd.y * qt, qo.z + qd.z * qt);
                        /* the unnormalised normal (rtcommon.h:389): written to LDS at the accept, the
                           same float operations on the same record (kept in registers instead it
                           measured 8 % slower, r01; a second fetch of the edges here is one more
                           dependent round trip per mesh hit) */
                        if (TRAV == RT_TRAV_BVH4Q) {
                            hn = v3(st_hn[0], st_hn[RT_BLOCK], st_hn[2 * RT_BLOCK]);
                        } else {
                            const float4 e1 = tris[3 * ts.best + 1];
                            const float4 e2 = tris[3 * ts.best + 2];
                            hn = cross3(v3(e2.x, e2.y, e2.z), v3(e1.x, e1.y, e1.z)); /* unnormalised, rtcommon.h:389 */
                        }
                        tri_hit = true;
                    } else {
                        if (SPLIT && depth == 0 && a.split_spec && a.split_which == RT_SPLIT_MESH &&
                            sample / a.split_chunk + 1u < a.split_chunks) {
                            /* a speculated pixel's camera ray missed the mesh: its later chunks started
                               from wrong seeds — listed once for the repair pass, which restarts at the
                               first such chunk (rare path) */
                            const uint32_t p = yl * a.W + x;
                            if (atomicMin(a.split_dirty + p, sample / a.split_chunk) == ~0u)
                                a.split_repair[(uint32_t)atomicAdd(a.counters + RT_CNT_REPAIR, 1ull)] = p;
                        }
                        /* the enclosing box (rtcommon.h:427-433); ray.tmax is still INF */
                        const float hd = intersect_box(qo, qd, RT_SMALL_F, bw, bh, bw);
                        if (hd > RT_SMALL_F && hd < kInf) {
                            hp = v3(qo.x + qd.x * hd, qo.y + qd.y * hd, qo.z + qd.z * hd);
                            hn = box_normal(hp, bw, bh, bw);
                            tri_hit = false;
                        } else {
                            surface = false;
                            sample_done = true; /* path terminates (rtcommon.h:463-466) */
                        }
                    }
                    if (surface) { /* sample_direct_illumination_tri, rtcommon.h:78-105 */
                        /* the shadow-ray origin (so) becomes the query origin */
                        qo = v3(hp.x + hn.x * RT_SMALL_F, hp.y + hn.y * RT_SMALL_F, hp.z + hn.z * RT_SMALL_F);
                        direct = v3(0.0f, 0.0f, 0.0f);
                        light = 0;
                        if (n_lights > 0) want_shadow = true;
                        else seg_done = true;
                    }
                } else {
                    ++cnt[1];
                    if (COUNT || RT_PLAIN_PIXEL_STATS) ++pix_q;
                    /* the shadow cache: an unoccluded answer from a mesh hit (-1, from the full traversal;
                       not the -2 of a ray answered without one) leaves the pixel no cut node to start at */
                    if (!RT_NO_SHADOW_CACHE && tri_hit && ts.best == -1) *st_entry = 0;
                    if (ts.best < 0) { /* unoccluded: rtcommon.h:93-101 */
                        const float cw = qd.x * hn.x + qd.y * hn.y + qd.z * hn.z;
                        if (cw > 0) {
                            direct.x += s_light[light * 8 + 4] * cw;
                            direct.y += s_light[light * 8 + 5] * cw;
                            direct.z += s_light[light * 8 + 6] * cw;
                        }
                    }
                    ++light;
                    if (light < n_lights) want_shadow = true;
                    else seg_done = true;
                }
                bool bounce = false;
                if (seg_done) {
                    const float scale = 1.0f * RT_M_1_PI_F;
                    V3 prop = v3(PROP_GET(0), PROP_GET(1), PROP_GET(2));
                    if (tri_hit) { /* rtcommon.h:411-421: no bounce off triangles */
                        col_x += prop.x * direct.x * scale * 0.7f;
                        col_y += prop.y * direct.y * scale * 0.7f;
                        col_z += prop.z * direct.z * scale * 0.7f;
                        sample_done = true;
                    } else { /* rtcommon.h:435-461: albedo 0.7, Lambert bounce (drawn even at the last depth) */
                        prop.x *= 0.7f;
                        prop.y *= 0.7f;
                        prop.z *= 0.7f;
                        col_x += prop.x * direct.x * scale;
                        col_y += prop.y * direct.y * scale;
                        col_z += prop.z * direct.z * scale;
                        PROP_SET(0, prop.x);
                        PROP_SET(1, prop.y);
                        PROP_SET(2, prop.z);
                        qo = hp;
                        bounce = true;
                    }
                }
                /* Next direction, light sample or Lambert bounce, through ONE code path: both
                   draw r1 then r2 (rtcommon.h:92, :459), build (cos(phi) st, sin(phi) st, ct)
                   with phi = 2 pi r2 and st = sqrt(1 - ct^2), and rotate it about an axis
                   (shading_to_world) — sphereEmissiveRadiance (materials.h:232-271) about the
                   direction to the light with ct = 1 + r1 (cos_max - 1), cos_sample_hemisphere
                   (materials.h:21-35) about the normal with ct = sqrt(1 - r1).  Only ct and the
                   axis differ, so lanes of both kinds share the sin/cos and the frame. */
                if (want_shadow || bounce) {
                    const float r1 = frand(seed);
                    const float r2 = frand(seed);
                    V3 axis = hn;
                    float ct = 0.0f;
                    V3 lc = hn;
                    float lr = 0.0f;
                    if (want_shadow) {
                        lc = v3(s_light[light * 8 + 0], s_light[light * 8 + 1], s_light[light * 8 + 2]);
                        lr = s_light[light * 8 + 3];
                        V3 dir = v3(lc.x - qo.x, lc.y - qo.y, lc.z - qo.z);
                        const float inv = rt_rsqrtf(dir.x * dir.x + dir.y * dir.y + dir.z * dir.z);
                        dir.x *= inv;
                        dir.y *= inv;
                        dir.z *= inv;
                        const float sin_max = lr * inv;
                        const float cos_max = rt_sqrtf(1.0f - sin_max * sin_max);
                        ct = 1.0f + r1 * (cos_max - 1.0f);
                        axis = dir;
                    } else {
                        ct = rt_sqrtf(1.0f - r1);
                    }
                    const float st = rt_sqrtf(1.0f - ct * ct);
                    const float phi = RT_M_2PI_F * r2;
                    float sphi, cphi;
                    rt_sincosf(phi, &sphi, &cphi);
                    qd = shading_to_world(v3(cphi * st, sphi * st, ct), axis);
                    if (want_shadow) {
                        stmax = intersect_sphere(qo, qd, RT_SMALL_F, lc, lr) - RT_SMALL_F;
                        mode = M_SHADOW;
                    } else {
                        ++depth;
                        if (depth > a.max_depth) sample_done = true;
                        else mode = M_CLOSEST;
                    }
                }
                if (SPLIT && sample_done) { /* the sample's radiance, summed in order by k_split_finish */
                    hit_depth = 0; /* read per task: its first sample's */
                    float *dst = a.split_col + ((size_t)sample * (a.W * a.Hl) + (yl * a.W + x)) * 3u;
                    dst[0] = col_x;
                    dst[1] = col_y;
                    dst[2] = col_z;
                    ++sample;
                    mode = (sample >= spp || sample % a.split_chunk == 0u) ? M_IDLE : M_NEWSAMPLE;
                    if (a.pixel_iter && mode == M_IDLE) /* the chunk task's finish */
                        a.pixel_iter[(size_t)a.W * a.Hl * a.split_chunks + (size_t)(yl * a.W + x) * a.split_chunks +
                                     (sample - 1u) / a.split_chunk] = (uint32_t)pix_steps;
                    if (sample >= spp && !a.split_seed_slot) /* the pixel's final seed, from its last chunk's own draws
                                                                (a slotted long chain's: from its seed pass) */
                        reinterpret_cast<uint2 *>(a.split_seed)[(size_t)(yl * a.W + x) * a.split_nseed + a.split_nseed - 1u] =
                            make_uint2(seed.x, seed.y);
                    if (mode == M_IDLE) {
                        pclass = -1;
                        if (COUNT && a.pixel_stats) { /* diagnostics: the pixel's queries and steps over its chunks */
                            uint32_t *ps = pixel_stats_rec(a, x, yl);
                            atomicAdd(ps + 5, (uint32_t)pix_q);
                            atomicAdd(ps + 6, (uint32_t)pix_steps);
                        }
                    }
                } else if (sample_done) {
                    ACC_SET(0, ACC_GET(0) + col_x);
                    ACC_SET(1, ACC_GET(1) + col_y);
                    ACC_SET(2, ACC_GET(2) + col_z);
                    ++sample;
                    mode = M_NEWSAMPLE;
                    if (sample >= spp) { /* raytracer.cl:234-242 */
                        write_pixel(out + ((size_t)yl * a.W + x),
                                    pixel_mean(ACC_GET(0), ACC_GET(1), ACC_GET(2), (float)spp), a.progressive > 0, mix_t);
                        store_seed(a, seed_slot(a, x, yl), seed.x, seed.y);
                        if (a.pixel_iter) a.pixel_iter[a.W * a.Hl + yl * a.W + x] = (uint32_t)pix_steps;
                        mode = M_IDLE;
                        pclass = -1;
                        if ((COUNT || RT_PLAIN_PIXEL_STATS) && a.pixel_stats) { /* diagnostics (RT_PIXEL_STATS) */
                            uint32_t *ps = pixel_stats_rec(a, x, yl);
                            ps[0] = pix_rt0;
                            ps[1] = (uint32_t)__builtin_amdgcn_s_memrealtime();
                            ps[2] = (COUNT || RT_PLAIN_PIXEL_STATS) ? (uint32_t)pix_q : 0u;
                            ps[3] = (COUNT || RT_PLAIN_PIXEL_STATS) ? (uint32_t)pix_steps : 0u;
                            ps[4] = (COUNT || RT_PLAIN_PIXEL_STATS) ? (uint32_t)(pix_d >> 6) : 0u;
                            ps[5] = (COUNT || RT_PLAIN_PIXEL_STATS) ? (uint32_t)(pix_ab >> 6) : 0u;
                            ps[6] = (COUNT || RT_PLAIN_PIXEL_STATS) ? (uint32_t)(pix_c >> 6) : 0u;
                            ps[7] = (COUNT || RT_PLAIN_PIXEL_STATS) ? (uint32_t)pix_it : 0u;
                        }
                        if (COUNT && !RT_DIAG_MIX && !RT_DIAG_RAYSPLIT && !RT_DIAG_SHCACHE && !RT_DIAG_INLINE) {
                            const unsigned long long dt = wave_clock() - pix_t0;
                            cnt[10] = dt > cnt[10] ? dt : cnt[10];
                            cnt[11] = pix_q > cnt[11] ? pix_q : cnt[11];
                            cnt[12] = pix_steps > cnt[12] ? pix_steps : cnt[12];
                        }
                    }
                }
            }
            /* a shadow ray just issued whose answer is known without a traversal (the C-phase rule
               below: tmax <= tmin, or cos(wi) <= 0) is answered here and the path advanced again in
               this pass, instead of after a whole stepping round (-3.9 %, profiles/r01n) */
            const float cw_q = qd.x * hn.x + qd.y * hn.y + qd.z * hn.z;
            const bool issued = mode == M_SHADOW && !fin && !running;
            const bool need_trav = stmax > RT_SMALL_F && cw_q > 0;
            /* likewise a long chain's box segment (split_hit_depth): no triangle accepted */
            const bool known_miss = SPLIT && mode == M_CLOSEST && !fin && !running && (int)depth < hit_depth;
            /* and a box-path query (a bounce off the box, or a shadow ray leaving it) whose segment misses
               the mesh's padded bounds: no triangle accepted, whatever the traversal would visit */
            bool off_mesh = false;
            if (!SPLIT && redo_pass < kOffMeshRedo && a.mesh_bounds && !tri_hit && !fin && !running &&
                ((mode == M_SHADOW && need_trav) || (mode == M_CLOSEST && depth > 0)))
                off_mesh = segment_misses_box(qo, qd, RT_SMALL_F, mode == M_SHADOW ? stmax : kInf, a.mesh_lo, a.mesh_hi);
            const bool redo = (issued && !need_trav) || known_miss || off_mesh;
            if (!__any(redo)) break;
            if (redo) {
                ts.best = -2; /* no hit, without a traversal */
                fin = true;
                ++cnt[RT_CNT_SKIPPED];
            }
        }

        const unsigned long long t_d1 = (COUNT || RT_PLAIN_PIXEL_STATS) ? wave_clock() : 0ull;
        if (COUNT) cnt[RT_CNT_SHADE] += t_d1 - t_d0;
        if (COUNT || RT_PLAIN_PIXEL_STATS) { /* (the plain launch's phase clocks: RT_PLAIN_PIXEL_STATS builds) */
            pix_d += t_d1 - t_d0;
            if (!INL || pass == 0) ++pix_it;
        }
        /* ---- A: refill idle lanes from the pixel queue (wave-private batches: one atomic per
                64 items; bunny class 1024^2 at 1 spp 0.95 -> 0.55 ms, the dragon frame +-0.5 %) ---- */
        const unsigned long long idle = __ballot(mode == M_IDLE);
        if (idle) {
            const uint32_t item = multi_q ? mq_take(a.work_counter, n_tasks, idle, bnext, bend, qs,
                                                    a.take_exact ? 0u : a.queue_batch,
                                                    SPLIT ? 64u * a.split_chunks : 64u)
                                          : batch_take(a.work_counter, idle, bnext, bend, a.take_exact ? 0u : kBatch);
            if (mode == M_IDLE) {
                if (multi_q && item == ~0u) {
                    if ((qs >> 8) >= RT_QHEADS) mode = M_DONE; /* else: idle, takes again next iteration */
                } else if (item >= n_tasks) {
                    mode = M_DONE;
                } else {
                    /* 8 x 8 pixel tiles, row-major over the (local) frame; SPLIT over tiles: a
                       tile's chunk 0 of its 64 pixels, then chunk 1, ... (the mesh pixels only when
                       the box pixels run apart: the 16 chunk layers of a tile run side by side,
                       10 % faster than layer after layer over the frame); SPLIT over the box
                       pixels: a pixel's chunks in turn */
                    uint32_t tile = item >> 6, chunk = 0;
                    const uint32_t in = item & 63u;
                    uint32_t sbase = 0; /* the task's seeds in split_seed (x split_nseed): its pixel or its long-chain slot */
                    bool take;
                    if (SPLIT && a.split_which == RT_SPLIT_BOX) {
                        const uint32_t slot = item / a.split_chunks;
                        chunk = item - slot * a.split_chunks;
                        const uint32_t p = a.split_box[a.split_item_base + slot];
                        x = p % a.W;
                        yl = p / a.W;
                        sbase = a.split_seed_slot ? slot : p;
                        /* a repaired pixel: its chunks before the first missed one stand */
                        take = !a.split_restart || chunk * a.split_chunk >= a.split_restart[p] * a.split_restart_chunk;
                    } else {
                        if (SPLIT) {
                            chunk = tile % a.split_chunks;
                            tile = tile / a.split_chunks;
                        }
                        take = tile_pixel(a, a.tile_order, tile, in, tiles_x, x, yl);
                        sbase = yl * a.W + x;
                        if (SPLIT && take && a.split_which == RT_SPLIT_MESH)
                            take = a.pixel_class[(size_t)yl * a.W + x] == -1;
                    }
                    if (RT_DIAG_ONE_PIXEL) { /* diagnostics build: the target pixel and the diag_k - 1 pixels
                                                after it in its 8 x 8 tile (in-tile order, wrapping) */
                        const uint32_t dx = a.diag_pixel % a.W, dy = a.diag_pixel / a.W;
                        const uint32_t in0 = (dy & 7u) * 8u + (dx & 7u);
                        take = take && (x >> 3) == (dx >> 3) && (yl >> 3) == (dy >> 3) && ((in - in0) & 63u) < a.diag_k;
                    }
                    if (take) s_list[threadIdx.x] = list_pack(a, x, yl, tiles_x);
                    if (!RT_NO_SHADOW_CACHE && take) *st_entry = 0; /* a pixel's (a chunk's) cache is its own */
                    if (SPLIT && take && a.split_spec && a.split_which == RT_SPLIT_MESH) {
                        /* a speculated mesh pixel: the chunk's first seed jumped ahead from the
                           frame seed (split_spec_draws numbers per sample before it) */
                        const Seed fs = load_seed(a, seed_slot(a, x, yl));
                        const uint32_t k = chunk * a.split_chunk * a.split_spec_draws;
                        seed.x = mwc_jump<36969u>(fs.x, k, a.split_spec_mul[2 * chunk]);
                        seed.y = mwc_jump<18000u>(fs.y, k, a.split_spec_mul[2 * chunk + 1]);
                    } else if (SPLIT && take) { /* the chunk's first seed, from the seed pass */
                        const uint2 sd = reinterpret_cast<const uint2 *>(
                            a.split_seed)[(size_t)sbase * a.split_nseed + chunk * a.split_chunk / a.split_fine];
                        seed.x = sd.x;
                        seed.y = sd.y;
                    }
                    if (SPLIT && take) {
                        if (a.pixel_iter) /* a mesh pixel's chunk task: its take (pixel_iter, whole pixels: below) */
                            a.pixel_iter[(size_t)(yl * a.W + x) * a.split_chunks + chunk] = 0u;
                        sample = chunk * a.split_chunk;
                        if (a.split_hit_depth) hit_depth = a.split_hit_depth[(size_t)sbase * spp + sample];
                        pclass = a.pixel_class ? a.pixel_class[(size_t)yl * a.W + x] : -1;
                        mode = M_NEWSAMPLE;
                        pix_q = pix_steps = 0;
                    } else if (take) {
                        seed = load_seed(a, seed_slot(a, x, yl));
                        if (a.pixel_iter) a.pixel_iter[yl * a.W + x] = 0u;
                        if ((COUNT || RT_PLAIN_PIXEL_STATS) && a.pixel_stats)
                            pix_rt0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
                        if (COUNT) pix_t0 = wave_clock();
                        pix_q = pix_steps = pix_d = pix_ab = pix_c = pix_it = 0;
                        ACC_SET(0, 0.0f);
                        ACC_SET(1, 0.0f);
                        ACC_SET(2, 0.0f);
                        sample = 0;
                        /* some of the probe's rays missed the mesh: box paths, long chains */
                        pclass = a.pixel_class ? a.pixel_class[(size_t)yl * a.W + x] : -1;
                        if (RT_DIAG_SKIP && (RT_DIAG_SKIP == 1 ? pclass != -1 : pclass == -1)) {
                            mode = M_IDLE; /* diagnostics builds: the mesh / box pixels alone (wrong frames) */
                            pclass = -1;
                        } else if (spp > 0) {
                            mode = M_NEWSAMPLE;
                        } else { /* no samples: 0/0 pixels, seeds untouched (raytracer.cl:234-242) */
                            write_pixel(out + ((size_t)yl * a.W + x), pixel_mean(0.0f, 0.0f, 0.0f, 0.0f),
                                        a.progressive > 0, mix_t);
                        }
                    }
                }
            }
        }
        if (!__any(mode != M_DONE)) break;

        /* ---- B: camera ray of a new sample (raytracer.cl:216-224; sx outer,
                sy inner, the x draw before the y draw) ---- */
        if (mode == M_NEWSAMPLE) {
            /* The inline list resolve (INL instantiations): the camera query of a pixel with a
               candidate list is started here as phase C starts it, and stepped up to inline_k
               records through the stepping loop's own step (trav_step: the one copy of the test,
               the accept rule with its tie read-back, the hit normal and the list's early end),
               before the wave's next stepping round.  A query that ends there — most do, DESIGN.md
               §4.3 — never enters the loop: the lane is `fin` and the advance runs another round
               for it; the others go on in phase C from the record they stand at. */
            const uint32_t lpack = s_list[threadIdx.x];
            /* (a long chain's box segment, split_hit_depth, is answered without a query as before) */
            const bool inl = INL && TRAV == RT_TRAV_BVH4Q && inline_k && pass < inline_passes && lpack < RT_LPACK_EMPTY &&
                             !(SPLIT && hit_depth > 0);
            camera_ray(a, seed, x, global_row(a, yl), sample / a.sample_rate, sample % a.sample_rate, hw, hh, qo,
                       qd);
            PROP_SET(0, 1.0f);
            PROP_SET(1, 1.0f);
            PROP_SET(2, 1.0f);
            col_x = col_y = col_z = 0.0f;
            depth = 0;
            mode = M_CLOSEST;
            if (INL && TRAV == RT_TRAV_BVH4Q && inline_k && __any(inl)) {
                if (inl) { /* the list as virtual leaves: its first block the cursor, the later ones stacked */
                    const ListRange lr = list_range(lpack);
                    trav_begin(ts, stk, qo, qd, kInf);
                    ts.node = list_leaves(lr.count, lr.first, [&](int v) { stk.push(v); });
                    running = true;
                }
                for (uint32_t i = 0; i < inline_k; ++i) {
                    if (inl && running) {
                        TravCounts tc = {0u, 0u, 0u};
                        if (trav_step<TRAV, COUNT>(nodes, tris, ts, stk, qo, qd, RT_SMALL_F, false, tc, false, st_hn,
                                                   RT_NO_SHADOW_CACHE ? nullptr : st_entry, sc_cut)) {
                            running = false;
                            fin = true;
                            if (COUNT && RT_DIAG_INLINE) ++cnt[10];
                        }
                        /* steps of the pixel's measured cost and tests of a counting launch like the
                           loop's; lane_slots (cnt[5]) stays the loop's */
                        count_step<COUNT>(cnt, pix_steps, tc);
                    }
                    if (!__any(inl && running)) break;
                }
                if (COUNT && RT_DIAG_INLINE && inl && running) ++cnt[11];
            }
            if (COUNT && RT_DIAG_INLINE && !inl && lpack < RT_LPACK_EMPTY) ++cnt[11];
        }
        if (INL && __any(fin)) {
            if (COUNT || RT_PLAIN_PIXEL_STATS) pix_ab += wave_clock() - t_d1; /* (the last round's: before phase C) */
            ++pass;
            goto advance;
        }

        /* ---- C: ray queries ---- */
        /* the waves that hold box pixels (the long serial chains that end the frame) issue
           at top priority (measured against graded priorities: DESIGN.md §5); scheduling only */
        if (__any(pclass != -1)) __builtin_amdgcn_s_setprio(3);
        else __builtin_amdgcn_s_setprio(0);
        const bool pending = (mode == M_CLOSEST || mode == M_SHADOW) && !running && !fin;
        if (RESUME) {
            if (pending) {
                const bool shadow = (mode == M_SHADOW);
                const float qt = shadow ? stmax : kInf;
                /* Shadow rays whose answer cannot change the pixel are not traversed:
                   tmax <= tmin (the sample missed the light) can hit nothing
                   (visibility_test_tri returns true), and with cos(wi) <= 0 the light's
                   term is dropped whatever the visibility (rtcommon.h:93-95 tests
                   cosWi > 0 after the visibility test; the ray is const there, and
                   both draws were already made).  Same pixel, same seeds. */
                if ((shadow && (!(qt > RT_SMALL_F) || !(qd.x * hn.x + qd.y * hn.y + qd.z * hn.z > 0))) ||
                    (SPLIT && !shadow && (int)depth < hit_depth) || /* a long chain's box segment */
                    (!SPLIT && a.mesh_bounds && !tri_hit && (shadow || depth > 0) && /* (short frames: never split) */
                     segment_misses_box(qo, qd, RT_SMALL_F, qt, a.mesh_lo, a.mesh_hi))) { /* off the mesh */
                    ts.best = -2; /* no hit, without a traversal */
                    fin = true; /* (counted below) */
                } else {
                    trav_begin(ts, stk, qo, qd, qt);
                    if (shadow) ts.node = (int)a.shadow_root; /* the shadow queries' tree */
                    if (shadow && tri_hit && sc_cut.n) { /* a try under the cached cut node; the root on its failure */
                        const uint32_t e = *st_entry;
                        if (e) {
                            ts.node = (int)(sc_cut.lo + e - 1u);
                            ts.best = RT_SC_TRYING;
                            if (COUNT && RT_DIAG_SHCACHE) ++cnt[10];
                        }
                    }
                    running = true;
                    if (!shadow && depth == 0) { /* a camera ray: the pixel's candidate list */
                        const uint32_t lpack = s_list[threadIdx.x];
                        if (lpack == RT_LPACK_EMPTY) {
                            running = false;
                            ts.best = -1;
                            fin = true;
                        } else if (lpack != RT_LPACK_NONE) {
                            const ListRange lr = list_range(lpack);
                            ts.node = list_leaves(lr.count, lr.first, [&](int v) { stk.push(v); });
                        }
                    }
                }
            }
            /* the answers without a traversal are counted here, from the block's outcome (a pending
               lane leaves it with best = -2 only that way), and not inside it: a 64-bit value changed
               under the block's exec mask — the counter, or a 0 / 1 to add to it — was spilled at the
               block's end before the mask was restored (counting instantiations built without SLP
               packing), and the lanes outside the block read back a stale slot */
            cnt[RT_CNT_SKIPPED] += (pending && ts.best == -2) ? 1ull : 0ull;
            const unsigned long long t_c0 = (COUNT || RT_PLAIN_PIXEL_STATS) ? wave_clock() : 0ull;
            if (COUNT || RT_PLAIN_PIXEL_STATS) pix_ab += t_c0 - t_d1;
            /* The exit threshold follows the wave's live queries: with few lanes left (the
               frame's tail, or a small tile) a fixed fetch_k is never reached, and every lane
               would wait for the wave's longest query before its path moves on — the long
               serial chains then run at the pace of their slowest neighbours. */
            int fetch_k = fetch_k_all;
            if (a.fetch_frac) {
                const int live = __popcll(__ballot(running || fin));
                const int k_live = (live * (int)a.fetch_frac + 63) >> 6;
                fetch_k = fetch_k < k_live ? fetch_k : (k_live > 1 ? k_live : 1);
            }
            for (;;) {
                /* RT_STEP_UNROLL steps per exit check (fewer wave-level ballots and branches) */
#pragma unroll
                for (int u = 0; u < RT_STEP_UNROLL; ++u) {
#if RT_DIAG_MIX
                    if (COUNT) { /* diagnostics build: wave-steps holding node and leaf lanes / nodes only / leaves only */
                        const unsigned long long bn = __ballot(running && ts.node >= 0), bl = __ballot(running && ts.node < 0);
                        if ((threadIdx.x & 63) == 0) {
                            cnt[10] += (bn && bl) ? 1u : 0u;
                            cnt[11] += (bn && !bl) ? 1u : 0u;
                            cnt[12] += (!bn && bl) ? 1u : 0u;
                        }
                    }
#endif
                    if (running) {
                        const bool shadow = (mode == M_SHADOW);
                        TravCounts tc = {0u, 0u, 0u};
                        const bool sc_try = COUNT && RT_DIAG_SHCACHE && ts.best == RT_SC_TRYING;
                        if (trav_step<TRAV, COUNT>(nodes, tris, ts, stk, qo, qd, RT_SMALL_F, shadow, tc,
                                                   shadow && tri_hit, st_hn, RT_NO_SHADOW_CACHE ? nullptr : st_entry,
                                                   sc_cut)) {
                            running = false;
                            fin = true;
                            if (COUNT && RT_DIAG_SHCACHE && sc_try) ++cnt[11]; /* (a try only ends a query occluded) */
                        }
                        count_step<COUNT>(cnt, pix_steps, tc);
                        if (COUNT && RT_DIAG_RAYSPLIT) {
                            const int k = shadow ? (tri_hit ? 10 : 11) : (depth == 0 ? 12 : -1);
                            if (k >= 0) cnt[k] += tc.nodes + tc.leaves;
                        }
                    }
                    if (COUNT) ++cnt[5];
                }
                if (!__any(running)) break;
                const unsigned long long fin_lanes = __ballot(fin);
                if (__popcll(fin_lanes) >= fetch_k) break;
            }
            if (COUNT || RT_PLAIN_PIXEL_STATS) {
                const unsigned long long dc = wave_clock() - t_c0;
                if (COUNT) cnt[6] += dc;
                pix_c += dc;
            }
        } else if (pending) {
            const bool shadow = (mode == M_SHADOW);
            ts.best_t = shadow ? stmax : kInf;
            ts.best = -1;
            TravCounts tc = {0u, 0u, 0u};
            if (!shadow || ts.best_t > RT_SMALL_F)
                ts.best = traverse<TRAV, COUNT>(nodes, tris, a.n_tris, qo, qd, RT_SMALL_F, ts.best_t, shadow, stk, tc);
            fin = true;
            if (COUNT) {
                cnt[2] += tc.nodes;
                cnt[3] += tc.tests;
            }
        }
    }
    if (COUNT) cnt[7] = wave_clock() - t_k0;
    flush_counters(a.counters, cnt, COUNT);
}
#undef ACC_GET
#undef ACC_SET
#undef PROP_GET
#undef PROP_SET

} // namespace

/* ======================================================================== */
/* The launch.  k_tris has 20 instantiations: the compressed 4-wide traversal (RT_TRAV_BVH4Q) in all
   16 combinations of COUNT, SPLIT, MQ and INL — the sample-split form, the multi-head queue's take
   and the inline list resolve each cost the others registers or time (SPLIT: a full frame 1 %), so
   each is compiled in only where a launch uses it — and the linear loop and the full-precision
   4-wide traversal, which have none of the three, plain and counting. */

typedef void (*TrisKernel)(RtTriLaunch);

/* entry i of the BVH4Q table: COUNT = bit 0 of i, SPLIT = bit 1, MQ = bit 2, INL = bit 3 */
template <size_t... I>
constexpr std::array<TrisKernel, sizeof...(I)> tris_bvh4q_table(std::index_sequence<I...>)
{
    return {{k_tris<RT_TRAV_BVH4Q, (I & 1) != 0, (I & 2) != 0, (I & 4) != 0, (I & 8) != 0>...}};
}
constexpr auto kTrisBvh4q = tris_bvh4q_table(std::make_index_sequence<16>{});

/* the instantiation of a launch; split, mq and inl count for RT_TRAV_BVH4Q only */
static TrisKernel tris_kernel(int trav, bool count, bool split, bool mq, bool inl)
{
    if (trav == RT_TRAV_BVH4Q) return kTrisBvh4q[(count ? 1 : 0) | (split ? 2 : 0) | (mq ? 4 : 0) | (inl ? 8 : 0)];
    if (trav == RT_TRAV_LINEAR) return count ? k_tris<RT_TRAV_LINEAR, true> : k_tris<RT_TRAV_LINEAR, false>;
    return count ? k_tris<RT_TRAV_BVH4, true> : k_tris<RT_TRAV_BVH4, false>;
}

int rt_launch_tris(const RtTriLaunch &a, int trav, bool count, int grid_blocks, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const bool q = trav == RT_TRAV_BVH4Q;
    /* the multi-head queue: its own instantiations (its take costs the others registers) */
    const bool mq = a.queue_batch && q && a.split_which != RT_SPLIT_BOX;
    /* the sample-split form only where it is used (its code costs a full frame 1 %) */
    const bool split = q && a.split_chunks;
    if (split) {
        /* the chunk tasks (queue cursor a.work_counter — or the multi-head queue's heads — reset here) */
        const size_t words = mq ? (size_t)RT_QSTRIDE * RT_QHEADS : 1u;
        const hipError_t e = hipMemsetAsync(a.work_counter, 0, words * sizeof(uint32_t), st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(tris_kernel(trav, count, split, mq, a.inline_k != 0), dim3((unsigned)grid_blocks), dim3(RT_BLOCK),
                       0, st, a);
    return (int)hipGetLastError();
}

int rt_tris_grid_blocks(int device, int trav, bool count, int form, int *blocks)
{
    /* the occupancy of the form's instantiation with one queue head and no inline resolve */
    int per_cu = 0;
    const int e = (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, tris_kernel(trav, count, form == RT_FORM_SPLIT, false, false), RT_BLOCK, 0);
    if (e) return e;
    int n_cu = 0;
    const hipError_t he = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device);
    if (he != hipSuccess) return (int)he;
    if (getenv("RT_DEBUG_LAUNCH"))
        fprintf(stderr, "[rtmi] occupancy: trav %d count %d per_cu %d n_cu %d (device %d, err %d)\n", trav, (int)count,
                per_cu, n_cu, device, e);
    if (per_cu < 1) per_cu = 1;
    *blocks = per_cu * n_cu;
    return 0;
}

/* The end of a render: its counters (n_cnt words) written straight into the host's pinned, mapped
   copy, and the counters and queue cursors (n_zero words from `dev`, the counters first) zeroed for
   the next render — one small kernel on the render's stream instead of a copy-engine transfer
   plus a fill at the next render's start.  `totals` (RT_COUNTER_WORDS + 1 words, device) keeps the
   context's running totals over renders, whose counters are otherwise overwritten render by
   render when renders are enqueued back to back (rt_counter_totals): sums for the summed counters
   and the repair count, maxima for the per-pixel maxima, the OR of the guard words, and the
   number of renders in the last word.  host == nullptr: totals only (the copy-engine path). */
__global__ __launch_bounds__(256) void k_counters_out(unsigned long long *__restrict__ dev,
                                                      unsigned long long *__restrict__ host,
                                                      unsigned long long *__restrict__ totals, uint32_t n_cnt,
                                                      uint32_t n_zero)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_cnt) {
        const unsigned long long v = dev[i];
        if (host) host[i] = v;
        if (totals) {
            if (i < RT_N_SUM_COUNTERS || i == RT_CNT_REPAIR) totals[i] += v;
            else if (i == RT_CNT_GUARD) totals[i] |= v;
            else totals[i] = totals[i] > v ? totals[i] : v;
        }
    }
    if (totals && i == 0) totals[RT_COUNTER_WORDS] += 1ull;
    if (i < n_zero) dev[i] = 0ull;
}

int rt_launch_counters_out(unsigned long long *dev, unsigned long long *host_mapped, unsigned long long *totals,
                           uint32_t n_cnt, uint32_t n_zero, void *stream)
{
    const uint32_t n = n_cnt > n_zero ? n_cnt : n_zero;
    hipLaunchKernelGGL(k_counters_out, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, dev, host_mapped,
                       totals, n_cnt, n_zero);
    return (int)hipGetLastError();
}
