/*
 * rt_kernel_util.h — what the render kernels' files share: rt_tris.hip (k_tris), rt_split.hip (the
 * sample-split seed passes and finish kernels), rt_spheres.hip (the sphere kernels), rt_lists.hip
 * (the camera-ray candidate lists) and rt_sched.hip (k_probe_cost).
 *
 *   build-time switches   the default of every -DNAME=VALUE the render kernels read, in one block
 *   uniform_f             a launch-uniform float in an SGPR
 *   batch_take, mq_take   the pixel queues' takes (one head, RT_QHEADS heads), kBatch
 *   box_items             the item count of an RT_SPLIT_BOX launch
 *   wave_clock, wave_sum, flush_counters   the device counters
 *   pixel_stats_rec       a pixel's record of the RT_PIXEL_STATS diagnostics
 *   camera_dir, global_row, camera_ray     a pixel's camera ray and frame row, a sample's ray
 *   tile_pixel            a queue item's tile and in-tile index to its pixel
 *   seed_slot, load_seed, store_seed       a pixel's frame seeds
 *   pixel_mean, write_pixel                a finished pixel: the mean, the progressive mix, the store
 *   list_pack, RT_LPACK_*, list_range      a pixel's candidate list in one word, and back
 *   mwc_jump              frand's generators advanced by k draws
 *
 * Only force-inlined functions and constants that two of those files use belong here; everything
 * has internal linkage, as in rt_traverse.h.  Private to csrc/.
 */
#ifndef RT_KERNEL_UTIL_H
#define RT_KERNEL_UTIL_H

#include <hip/hip_runtime.h>

#include "rt_device.h"
#include "rt_internal.h"

#pragma clang fp contract(off)

/* ---- build-time switches of the render kernels (make EXTRA=-DNAME=VALUE) ----
   RT_STACK_DEPTH, RT_STEP_UNROLL, RT_TRIS_WAVES, RT_QHEADS, RT_QSTRIDE, RT_LIST_MAX and the
   diagnostics RT_DIAG_ONE_PIXEL / RT_PLAIN_PIXEL_STATS are read by host code too: rt_internal.h. */
/* k_tris (rt_tris.hip): diagnostics and A/B builds */
#ifndef RT_DIAG_RAYSPLIT
#define RT_DIAG_RAYSPLIT 0 /* diagnostics build: counting launches sum the stepping loop's steps of shadow rays
                              from mesh hits / shadow rays from the box / camera rays into counters 10 / 11 / 12 */
#endif
#ifndef RT_DIAG_SHCACHE
#define RT_DIAG_SHCACHE 0 /* diagnostics build: counting launches sum the shadow cache's tries / the tries that
                             answered (rt_traverse.h ShadowCut) into counters 10 / 11 */
#endif
#ifndef RT_DIAG_INLINE
#define RT_DIAG_INLINE 0 /* diagnostics build: counting launches sum the camera queries of listed pixels that k_tris's
                            phase B resolved inline / handed to the stepping loop into counters 10 / 11 */
#endif
#ifndef RT_NO_SHADOW_CACHE
#define RT_NO_SHADOW_CACHE 0 /* A/B build: k_tris without the shadow cache's code (RT_SHADOW_CACHE=0 only empties the cut) */
#endif
#ifndef RT_DIAG_MIX
#define RT_DIAG_MIX 0 /* diagnostics build (profiles/step_mix.py): counting launches report the stepping
                         rounds' wave-step mix in the per-pixel-maximum counters */
#endif
#ifndef RT_DIAG_SKIP
#define RT_DIAG_SKIP 0 /* diagnostics builds: k_tris skips the box pixels (1) or the mesh pixels (2) */
#endif
/* the 1- and 4-lane seed pass (rt_split.hip seed_pass) */
#ifndef RT_SEED_STATS
#define RT_SEED_STATS 0 /* diagnostics builds: per-pixel query / immediate-answer / iteration counts (RT_PIXEL_STATS) */
#endif
#ifndef RT_SEED_UNROLL
#define RT_SEED_UNROLL 4 /* seed-pass traversal steps per loop iteration */
#endif
#ifndef RT_SEED_IMM
#define RT_SEED_IMM 2 /* path-advance passes per seed-pass iteration (queries answered at once chain) */
#endif
/* the subtree-parallel seed pass (rt_split.hip k_chain_seeds) */
#ifndef RT_CHAIN_IMM
#define RT_CHAIN_IMM 2 /* path-advance passes per iteration */
#endif
#ifndef RT_CHAIN_UNROLL
#define RT_CHAIN_UNROLL 3 /* traversal steps per iteration (1 / 2 / 3 / 4: 8-way tile 16.8 / 16.4 / 16.3 / 16.4 ms, r04h2) */
#endif
/* the sphere kernels (rt_spheres.hip k_spheres) */
#ifndef RT_SPH_TILE
#define RT_SPH_TILE 16 /* pixel tile per block, RT_SPH_TILE^2 threads (A/B: 8) */
#endif

namespace {

/* a launch-uniform float held in an SGPR */
__device__ __forceinline__ float uniform_f(float v)
{
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

/* Queue items for a wave's idle lanes (ranked by a prefix popcount of the idle ballot) from a
   wave-private batch of kBatch consecutive items: one atomicAdd per batch instead of one per
   refill.  A single head word saturates at about 88 dequeues per microsecond
   (MI355X_MICROARCH.md, dequeue), which the many short tasks of a sample-split launch exceed.
   Wave-uniform: call with every lane active; bnext / bend start equal; batch >= the takers
   per wave (k <= batch).  batch 0: exactly the items the idle lanes need, none held back — for
   queues of long tasks (many-sample whole pixels), where a batch held by a wave whose lanes are
   busy starts its last items late: the dragon frame's last tile started ~9 ms after the queue
   ran dry (profiles/r05r), and at ~20 dequeues per microsecond one atomic per refill is cheap. */
constexpr uint32_t kBatch = 64;

__device__ __forceinline__ uint32_t batch_take(uint32_t *counter, unsigned long long idle, uint32_t &bnext,
                                               uint32_t &bend, uint32_t batch = kBatch)
{
    const uint32_t k = (uint32_t)__popcll(idle);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
    const uint32_t avail = bend - bnext;
    const uint32_t from_b = k < avail ? k : avail;
    uint32_t nb = 0;
    const uint32_t take = batch ? batch : k - from_b;
    if (k > from_b) {
        const int leader = __ffsll((long long)idle) - 1;
        if ((int)(threadIdx.x & 63) == leader) nb = atomicAdd(counter, take);
        nb = __builtin_amdgcn_readfirstlane(__shfl(nb, leader));
    }
    const uint32_t item = rank < from_b ? bnext + rank : nb + (rank - from_b);
    if (k > from_b) {
        bnext = nb + (k - from_b);
        bend = nb + take;
    } else {
        bnext += k;
    }
    return item;
}

/* Multi-head queue (RT_QHEADS heads, RT_QSTRIDE words apart): a launch's items are 64-item groups
   (an 8 x 8 tile, or one chunk layer of a tile); head h owns the groups g = h, h + RT_QHEADS, ...
   (in queue order), and a wave takes `batch` items of a head at a time, starting at the head of
   its block (blockIdx.x mod RT_QHEADS) and moving on to the next head when one is drained.  More
   heads take more dequeues per microsecond than one (a single head word saturates near 88), so
   the batches can be small enough that no wave holds back many of the queue's last items while
   its lanes are busy.  The wave's state is one word `qs`: the head of its batch [bnext, bend)
   (local indices, bits 0-3), the head it takes from next (bits 4-7), and how many heads in a row
   it found drained (bits 8-11: RT_QHEADS of them, the queue is empty).  At most one atomic per
   take; a lane whose take found a drained head stays idle and takes again in the next iteration.
   Returns the lane's item or ~0u.  Wave-uniform, like batch_take. */
__device__ __forceinline__ uint32_t mq_take(uint32_t *heads, uint32_t n_tasks, unsigned long long idle, uint32_t &bnext,
                                            uint32_t &bend, uint32_t &qs, uint32_t batch, uint32_t span = 64u)
{
    constexpr uint32_t Q = RT_QHEADS;
    const uint32_t k = (uint32_t)__popcll(idle);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
    const uint32_t avail = bend - bnext;
    const uint32_t from_b = k < avail ? k : avail;
    const uint32_t bq = qs & 15u, hq = (qs >> 4) & 15u;
    /* local index l of head q -> queue item: span-item group (l / span) x Q + q, offset l mod span (span
       64: a tile; a split launch's 64 x chunks: a tile's chunk layers together) */
    auto global = [&](uint32_t l, uint32_t q) { return ((l / span) * Q + q) * span + l % span; };
    uint32_t item = rank < from_b ? global(bnext + rank, bq) : ~0u;
    bnext += from_b;
    if (k > from_b && (qs >> 8) < Q) {
        const int leader = __ffsll((long long)idle) - 1;
        uint32_t nb = 0;
        const uint32_t take = batch ? batch : k - from_b; /* batch 0: exactly the items needed */
        if ((int)(threadIdx.x & 63) == leader) nb = atomicAdd(heads + RT_QSTRIDE * hq, take);
        nb = __builtin_amdgcn_readfirstlane(__shfl(nb, leader));
        const uint32_t n_groups = n_tasks / span;
        const uint32_t n_local = (n_groups > hq ? (n_groups - hq + Q - 1u) / Q : 0u) * span;
        if (nb < n_local) {
            const uint32_t r = rank - from_b;
            bend = nb + take < n_local ? nb + take : n_local;
            if (rank >= from_b && nb + r < bend) item = global(nb + r, hq);
            const uint32_t need = k - from_b;
            bnext = nb + (need < bend - nb ? need : bend - nb);
            qs = hq | hq << 4; /* the batch's head, the same head next, no drained heads */
        } else { /* drained: the next head, one more drained in a row */
            qs = (qs & 15u) | ((hq + 1u) % Q) << 4 | ((qs >> 8) + 1u) << 8;
        }
    }
    return item;
}

/* RT_SPLIT_BOX launches: the number of items of split_box[split_item_base ...] this launch takes
   (the list's length from the device when split_n_dev is set), at most split_item_cap */
__device__ __forceinline__ uint32_t box_items(const RtTriLaunch &a)
{
    const uint32_t n = a.split_n_dev ? *a.split_n_dev : a.split_n_box;
    const uint32_t m = n > a.split_item_base ? n - a.split_item_base : 0u;
    return a.split_item_cap && m > a.split_item_cap ? a.split_item_cap : m;
}

/* shader-clock timestamp (s_memtime), counting launches only */
__device__ __forceinline__ unsigned long long wave_clock()
{
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ void flush_counters(unsigned long long *dst, const unsigned long long (&v)[RT_N_COUNTERS],
                                               bool with_trav)
{
    for (int i = 0; i < RT_N_SUM_COUNTERS; ++i) {
        if (!with_trav && i >= 2 && i != RT_CNT_SKIPPED) continue;
        const unsigned long long w = wave_sum(v[i]);
        if ((threadIdx.x & 63) == 0) atomicAdd(&dst[i], w);
    }
    if (with_trav) /* per-pixel maxima (RT_DIAG_MIX builds: the wave-step mix, summed) */
        for (int i = RT_N_SUM_COUNTERS; i < RT_N_COUNTERS; ++i) {
            if (RT_DIAG_MIX || RT_DIAG_RAYSPLIT || RT_DIAG_SHCACHE || RT_DIAG_INLINE) atomicAdd(&dst[i], v[i]);
            else atomicMax(&dst[i], v[i]);
        }
}

/* pixel (x, yl)'s 8-word record of the RT_PIXEL_STATS diagnostics */
__device__ __forceinline__ uint32_t *pixel_stats_rec(const RtTriLaunch &a, uint32_t x, uint32_t yl)
{
    return a.pixel_stats + 8 * ((size_t)yl * a.W + x);
}

/* raytracer.cl:81-85: normalize(view + right*a + up*b), float4 lanes incl. w,
   normalize pinned as v / sqrt(dot(v, v)). */
__device__ __forceinline__ V3 camera_dir(const rt_camera &cam, float a, float b)
{
    const float x = (cam.view.x + cam.right.x * a) + cam.up.x * b;
    const float y = (cam.view.y + cam.right.y * a) + cam.up.y * b;
    const float z = (cam.view.z + cam.right.z * a) + cam.up.z * b;
    const float w = (cam.view.w + cam.right.w * a) + cam.up.w * b;
    const float len = rt_sqrtf(((x * x + y * y) + z * z) + w * w);
    return v3(x / len, y / len, z / len);
}

/* The frame row of a tile's row yl: the interleaved partition's formula, or the owner map's stripe
   list (rt_tile.stripe_owner; only a frame's last stripe can be short, and it is its owner's last) */
template <class L>
__device__ __forceinline__ uint32_t global_row(const L &a, uint32_t yl)
{
    if (a.stripe_map) return a.stripe_map[yl / a.stripe] * a.stripe + yl % a.stripe;
    if (a.n_ranks <= 1) return yl;
    return ((yl / a.stripe) * a.n_ranks + a.rank) * a.stripe + (yl % a.stripe);
}

/* The camera ray of sample (sx, sy) of the pixel in column x of frame row y (global_row)
   (raytracer.cl:216-224: sx outer, sy inner, the x draw before the y draw); hw, hh: half the frame's
   width and height */
template <class L>
__device__ __forceinline__ void camera_ray(const L &a, Seed &seed, uint32_t x, uint32_t y, uint32_t sx, uint32_t sy,
                                           float hw, float hh, V3 &o, V3 &d)
{
    const float fa = (float)x + strat_rand(seed, (int)sx, (int)a.sample_rate);
    const float fb = (float)y + strat_rand(seed, (int)sy, (int)a.sample_rate);
    o = v3(a.cam.position.x, a.cam.position.y, a.cam.position.z);
    d = camera_dir(a.cam, fa - hw, fb - hh);
}

/* Pixel `in` (row-major) of 8 x 8 tile `tile` (position `tile` of the queue's order, when there is
   one) of a frame tiles_x tiles wide; false outside the frame */
template <class L>
__device__ __forceinline__ bool tile_pixel(const L &a, const uint32_t *order, uint32_t tile, uint32_t in,
                                           uint32_t tiles_x, uint32_t &x, uint32_t &yl)
{
    if (order) tile = order[tile];
    x = (tile % tiles_x) * 8u + (in & 7u);
    yl = (tile / tiles_x) * 8u + (in >> 3);
    return x < a.W && yl < a.Hl;
}

/* A pixel's frame seeds: words `slot` and plane + `slot` of a.seeds (raytracer.cl:207-209, :241-242:
   the unshifted slot of its frame row) */
template <class L>
__device__ __forceinline__ uint32_t seed_slot(const L &a, uint32_t x, uint32_t yl)
{
    return global_row(a, yl) * a.Wpad + x;
}
template <class L>
__device__ __forceinline__ Seed load_seed(const L &a, uint32_t slot)
{
    const Seed s = {a.seeds[slot], a.seeds[a.Wpad * a.Hpad + slot]};
    return s;
}
template <class L>
__device__ __forceinline__ void store_seed(const L &a, uint32_t slot, uint32_t sx, uint32_t sy)
{
    a.seeds[slot] = sx;
    a.seeds[a.Wpad * a.Hpad + slot] = sy;
}

/* A finished pixel (raytracer.cl:234-242): the mean of its n samples' sum (0 / 0 without samples),
   then mixed into the frame's pixel by t = 1 / progressive when `mix` (progressive > 0), and stored */
__device__ __forceinline__ float4 pixel_mean(float sx, float sy, float sz, float n)
{
    return make_float4(sx / n, sy / n, sz / n, 0.0f / n);
}
__device__ __forceinline__ void write_pixel(float4 *dst, float4 p, bool mix, float t)
{
    if (mix) {
        const float4 old = *dst;
        p.x = old.x + (p.x - old.x) * t;
        p.y = old.y + (p.y - old.y) * t;
        p.z = old.z + (p.z - old.z) * t;
        p.w = old.w + (p.w - old.w) * t;
    }
    *dst = p;
}

/* A pixel's camera-ray candidate list (k_pixel_lists) packed in one word, read when the lane takes
   the pixel instead of before every sample's camera query (one dependent load less per sample):
   (first slot / 8) << RT_LIST_BITS | (count - 1) — lists start on 8-record multiples and slots stay
   below 2^28 (rt_render.cpp list_cap), so the word stays below RT_LPACK_EMPTY. */
constexpr uint32_t RT_LPACK_NONE = 0xffffffffu, RT_LPACK_EMPTY = 0xfffffffeu;
__device__ __forceinline__ uint32_t list_pack(const RtTriLaunch &a, uint32_t x, uint32_t yl, uint32_t tiles_x)
{
    if (!a.list_code) return RT_LPACK_NONE;
    const uint32_t code = a.list_code[yl * a.W + x];
    const uint32_t block = a.list_tile[(yl >> 3) * tiles_x + (x >> 3)];
    if (code == RT_LIST_NONE) return RT_LPACK_NONE;
    if (code == RT_LIST_EMPTY) return RT_LPACK_EMPTY;
    const uint32_t first = block + ((code >> RT_LIST_BITS) << 3);
    return ((first >> 3) << RT_LIST_BITS) | (code & (RT_LIST_MAX - 1u));
}
/* ... and back: the list's record count and first slot (of a word below RT_LPACK_EMPTY) */
struct ListRange {
    uint32_t count, first;
};
__device__ __forceinline__ ListRange list_range(uint32_t lpack)
{
    const ListRange r = {(lpack & (RT_LIST_MAX - 1u)) + 1u, (lpack >> RT_LIST_BITS) << 3};
    return r;
}

/* One MWC generator of frand (rng.h:9-47: x = A (x & 0xffff) + (x >> 16)) advanced by k draws.
   With M = A 2^16 - 1 the step is x -> A x mod M on the states below M (the step keeps them
   there; a fresh seed at or above M gets there within 2 steps, M itself is a fixed point), so
   k draws are one multiplication by A^k mod M (`mul`, from the host); a^-1 = 2^16 mod M undoes
   the canonicalising steps.  Small k: the steps themselves. */
template <uint32_t A>
__device__ __forceinline__ uint32_t mwc_jump(uint32_t x, uint32_t k, uint32_t mul)
{
    constexpr uint32_t M = A * 65536u - 1u;
    if (k <= 16u) {
        for (uint32_t i = 0; i < k; ++i) x = A * (x & 65535u) + (x >> 16);
        return x;
    }
    uint32_t k0 = 0;
    while (x > M) { /* at most 2 steps (every 32-bit state checked) */
        x = A * (x & 65535u) + (x >> 16);
        ++k0;
    }
    if (x == M) return M;
    for (uint32_t i = 0; i < k0; ++i) mul = (uint32_t)(((unsigned long long)mul * 65536u) % M);
    return (uint32_t)(((unsigned long long)x * mul) % M);
}

} // namespace

#endif /* RT_KERNEL_UTIL_H */
