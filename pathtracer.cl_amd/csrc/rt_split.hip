/*
 * rt_split.hip — the kernels around k_tris in a sample-split render: a
 * pixel's random numbers depend only on its closest hits, so a seed pass walks its samples with
 * the closest-hit queries alone and stores the seed each chunk of samples starts from; k_tris
 * (rt_tris.hip) renders the chunks as independent tasks; a finish kernel adds the samples'
 * radiance in sample order.
 *
 *   k_split_seeds<1 / 4>    seed_pass: one lane per chain (trav_step_q), or the 4-lane cooperative
 *                           query with a shared LDS stack (coop_round, the quad_* DPP exchanges)
 *   k_chain_seeds<G, RUNS>  the subtree-parallel pass of the long chains, G = 8 .. 64 lanes per
 *                           chain over a cut of the tree (chain_cut, edge_hit, group_box);
 *                           RUNS: the repair pass of speculated pixels
 *   k_split_finish, k_split_finish_list   the in-order sums: every pixel / a wave per listed pixel
 *   rt_launch_split_seeds, rt_launch_split_finish   rt_launch_split_seeds chooses among both seed
 *                           passes, which is why they share a file
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rt_device.h"
#include "rt_internal.h"
#include "rt_quant.h"
#include "rt_traverse.h"
#include "rt_kernel_util.h"

#pragma clang fp contract(off)

namespace {

/* Cooperative queries of the long chains' seed pass (coop_round below): the 4 lanes of a group
   (lanes 4g..4g+3 of a wave) advance ONE query together, its stack in LDS (RT_COOP_STACK entries
   per group).  Quad (4-lane group) exchanges through DPP quad_perm: a VALU modifier, not an LDS round trip
   like ds_bpermute (__shfl), whose latency a lone chain's wave cannot hide */
template <int CTRL>
__device__ __forceinline__ int quad_dpp(int v)
{
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, false);
}
template <int M> /* the value of lane sub ^ M */
__device__ __forceinline__ int quad_xor(int v)
{
    return M == 1 ? quad_dpp<0xB1>(v) : M == 2 ? quad_dpp<0x4E>(v) : quad_dpp<0x1B>(v);
}
__device__ __forceinline__ float quad_xorf1(float v) { return __int_as_float(quad_xor<1>(__float_as_int(v))); }
__device__ __forceinline__ float quad_xorf2(float v) { return __int_as_float(quad_xor<2>(__float_as_int(v))); }
/* the value of quad lane k (k uniform within the quad) */
__device__ __forceinline__ int quad_bcast(int v, int k)
{
    const int b0 = quad_dpp<0x00>(v), b1 = quad_dpp<0x55>(v), b2 = quad_dpp<0xAA>(v), b3 = quad_dpp<0xFF>(v);
    return k == 0 ? b0 : k == 1 ? b1 : k == 2 ? b2 : b3;
}

/* The 4-lane group's stack in the block's LDS stack area, inside the words its wave's lanes own
   in the per-lane layout ([depth][lane], RT_BLOCK words per depth): entry e of group g of wave w
   is word RT_BLOCK * (e / 4) + 64 w + 4 g + e % 4 (2-way bank conflicts between the groups). */
template <int G>
struct CoopStackG {
    static constexpr int kCap = RT_STACK_DEPTH * G; /* entries: the group's words of its wave's columns */
    lds_int *base; /* word 64 w + G g */
    __device__ __forceinline__ lds_int &operator[](int e) const
    {
        e = e < 0 ? 0 : e >= kCap ? kCap - 1 : e; /* never outside the group's words */
        return base[RT_BLOCK * (e / G) + (e % G)];
    }
};
typedef CoopStackG<4> CoopStack;

struct CoopQuery {
    int best, best_orig, sp;
    float best_t;
    V3 inv, oi;
};

__device__ __forceinline__ void coop_begin(CoopQuery &q, V3 o, V3 d, float tmax)
{
    q.inv = v3(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
    q.oi = v3(o.x * q.inv.x, o.y * q.inv.y, o.z * q.inv.z);
    q.best = -1;
    q.best_orig = -1;
    q.best_t = tmax;
    q.sp = 0;
}


/* Cooperative closest-hit query, one stack ITEM per lane: each round the 4 lanes of a group take
   the top entries of the group's stack — a node (one lane: its 4 child boxes) or the triangles of
   a leaf or candidate-list block (one lane each) — so a round tests up to 4 records of different
   subtrees instead of one node's boxes (scripts/sim_group_trav.cpp on box-path queries: 3.2
   rounds per closest-hit query, against 4.9 one-record steps).  The closest hit is order-free
   (minimum t, ties to the highest original index), so taking entries out of depth-first order
   changes only the work; a sorted candidate list's early end takes the bound of the last record
   tested, the latest in list order.  The group's whole query is on its stack (q.sp entries: the
   root, or the list blocks, pushed at the start); the item assignment is computed alike in the
   4 lanes.  Above `multi_sp` entries a round takes ONE item: 4 nodes add at most 12 entries, and
   a one-item depth-first walk from there at most the tree's worst stack (rt_render.cpp), so the
   stack stays inside the group's RT_COOP_STACK words. */
__device__ __forceinline__ bool coop_round(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                           CoopQuery &q, const CoopStack &gst, V3 o, V3 d, float tmin,
                                           uint32_t n_nodes, uint32_t n_recs, int multi_sp, unsigned long long *guard)
{
    const int lane = (int)(threadIdx.x & 63), sub = lane & 3, gbase = lane & ~3;
    if (q.sp <= 0) return true;
    const int L = q.sp <= multi_sp ? 4 : 1; /* lanes taking items this round */
    int e[4], cu[5];
    cu[0] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        e[j] = gst[q.sp - 1 - j]; /* read past the bottom: slot 0, unused */
        /* entry j (from the top) takes one lane if a node, one per triangle if a leaf */
        const int dm = j >= q.sp ? 0 : e[j] >= 0 ? 1 : (int)(~(uint32_t)e[j] & 7u) + 1;
        cu[j + 1] = cu[j] + dm;
    }
    /* branch-free, alike in the 4 lanes: lane `sub` takes entry j with cu[j] <= sub < cu[j+1]; the
       entries with cu[j+1] <= L are taken whole, and a leaf only partly taken stays on the stack
       with its first triangles removed */
    const int n_act = cu[4] < L ? cu[4] : L; /* lanes 0 .. n_act - 1 hold an item */
    const bool act = sub < n_act;
    const int j = (sub >= cu[1] ? 1 : 0) + (sub >= cu[2] ? 1 : 0) + (sub >= cu[3] ? 1 : 0);
    const int item = j == 0 ? e[0] : j == 1 ? e[1] : j == 2 ? e[2] : e[3];
    const int off = sub - (j == 0 ? 0 : j == 1 ? cu[1] : j == 2 ? cu[2] : cu[3]);
    const int top = q.sp < 4 ? q.sp : 4;
    int nfull = (cu[1] <= L ? 1 : 0) + (cu[2] <= L ? 1 : 0) + (cu[3] <= L ? 1 : 0) + (cu[4] <= L ? 1 : 0);
    nfull = nfull < top ? nfull : top;
    const int cp = nfull == 0 ? 0 : nfull == 1 ? cu[1] : nfull == 2 ? cu[2] : cu[3];
    const bool partial = nfull < top && cp < L;
    const int ep = nfull == 0 ? e[0] : nfull == 1 ? e[1] : nfull == 2 ? e[2] : e[3];
    const uint32_t used = (uint32_t)(L - cp), enp = ~(uint32_t)ep;
    const int part = ~(int)((((enp >> 3) + used) << 3) | ((enp & 7u) - used));
    /* the partly taken leaf's rest goes back now, in place (below every push of this round), so
       that nothing of the assignment stays live across the round but nfull */
    if (partial && sub == 0) gst[q.sp - 1 - nfull] = part;
    const bool leaf = item < 0;
    const uint32_t slot = (~(uint32_t)item >> 3) + (uint32_t)off;
    /* every record index is checked: a defect ends the query instead of reading outside the tree,
       and is reported (the render then fails: rt_synchronize) */
    const bool bad = act && (leaf ? slot >= n_recs : (uint32_t)item >= n_nodes);
    if ((__ballot(bad) >> gbase) & 15ull) {
        if (sub == 0) atomicOr(guard, (unsigned long long)RT_GUARD_INDEX); /* rare path: no register carried */
        return true;
    }
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    v4u w0 = {0u, 0u, 0u, 0u}, w1 = w0, w2 = w0, w3 = w0;
    if (act) {
        const v4u *vrec = reinterpret_cast<const v4u *>(leaf ? reinterpret_cast<const uint4 *>(tris) + 3 * slot
                                                             : reinterpret_cast<const uint4 *>(nodes) + 4 * item);
        w0 = vrec[0];
        w1 = vrec[1];
        w2 = vrec[2];
        if (!leaf) w3 = vrec[3];
    }
    asm volatile("" : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3));
    float ct = kInf, lbound = 0.0f;
    int co = -1, cs = -1, nh = 0;
    float t[4];
    int c[4];
    if (act && leaf) {
        const float4 ta = make_float4(__uint_as_float(w0.x), __uint_as_float(w0.y), __uint_as_float(w0.z),
                                      __uint_as_float(w0.w));
        const float4 tb = make_float4(__uint_as_float(w1.x), __uint_as_float(w1.y), __uint_as_float(w1.z), 0.0f);
        const float4 tc = make_float4(__uint_as_float(w2.x), __uint_as_float(w2.y), __uint_as_float(w2.z), 0.0f);
        float tt = 0.0f;
        const bool h = mt_test(o, d, ta, tb, tc, tt);
        const int orig = __float_as_int(ta.w);
        if (h && !(tt < tmin) && (tt < q.best_t || (tt == q.best_t && orig > q.best_orig))) {
            ct = tt;
            co = orig;
            cs = (int)slot;
        }
        lbound = __uint_as_float(w1.w); /* a list record: the next candidate's bound (tree leaves: 0) */
    } else if (act) {
        const uint4 q0 = make_uint4(w0.x, w0.y, w0.z, w0.w), q1 = make_uint4(w1.x, w1.y, w1.z, w1.w);
        const uint4 q2 = make_uint4(w2.x, w2.y, w2.z, w2.w), q3 = make_uint4(w3.x, w3.y, w3.z, w3.w);
        nh = node_children(q0, q1, q2, q3, q.inv, q.oi, d, q.best_t, false, false, t, c);
    }
    /* the group's best candidate: minimum t, ties to the highest original index */
    {
        const float ot = quad_xorf1(ct);
        const int oo = quad_xor<1>(co), os = quad_xor<1>(cs);
        const bool take = os >= 0 && (cs < 0 || ot < ct || (ot == ct && oo > co));
        ct = take ? ot : ct;
        co = take ? oo : co;
        cs = take ? os : cs;
    }
    {
        const float ot = quad_xorf2(ct);
        const int oo = quad_xor<2>(co), os = quad_xor<2>(cs);
        const bool take = os >= 0 && (cs < 0 || ot < ct || (ot == ct && oo > co));
        ct = take ? ot : ct;
        co = take ? oo : co;
        cs = take ? os : cs;
    }
    if (cs >= 0) {
        q.best = cs;
        q.best_t = ct;
        q.best_orig = co;
    }
    if (q.best_t < __int_as_float(quad_bcast(__float_as_int(lbound), n_act - 1))) return true;
    /* the stack: the taken entries off, a partly taken leaf back on top, then each node lane's hit
       children (lane 0's on top, each lane's nearest child last) */
    const int h1 = quad_dpp<0x55>(nh), h2 = quad_dpp<0xAA>(nh), h3 = quad_dpp<0xFF>(nh);
    const int total = quad_dpp<0x00>(nh) + h1 + h2 + h3;
    const int above = (sub < 1 ? h1 : 0) + (sub < 2 ? h2 : 0) + (sub < 3 ? h3 : 0);
    const int sp = q.sp - nfull;
    if (sp + total > CoopStack::kCap) { /* cannot happen (multi_sp bound, rt_render.cpp): reported, not clamped */
        if (sub == 0) atomicOr(guard, (unsigned long long)RT_GUARD_STACK);
        return true;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < nh) gst[sp + above + nh - 1 - i] = c[i];
    q.sp = sp + total;
    return q.sp == 0;
}

/* A cooperative query of the tree starts at the root's children: the root node (uniform, loaded
   once per wave into registers) is tested in the path advance instead of in a stepping round of
   its own, and the hit children go on the group's stack, nearest on top.  Returns false when no
   child box is hit (or the determinant cull rules the tree out): no mesh hit, without a round.
   Culling only: the same children coop_round would push from the root. */
__device__ __forceinline__ bool coop_root(uint4 r0, uint4 r1, uint4 r2, uint4 r3, CoopQuery &q, const CoopStack &gst, V3 d,
                                          bool writer)
{
    float t[4];
    int c[4];
    const int nh = node_children(r0, r1, r2, r3, q.inv, q.oi, d, q.best_t, false, false, t, c);
    if (writer) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nh) gst[nh - 1 - i] = c[i];
    }
    q.sp = nh;
    return nh > 0;
}

/* The same for a one-lane query (trav_step_q's state): the root's hit children go on the lane's
   stack, the nearest becomes the next node.  Returns false when none is hit. */
__device__ __forceinline__ bool lane_root(uint4 r0, uint4 r1, uint4 r2, uint4 r3, TravState &s, Stack &stk, V3 d)
{
    float t[4];
    int c[4];
    const int nh = node_children(r0, r1, r2, r3, s.inv, s.oi, d, s.best_t, false, false, t, c);
    if (nh >= 4) stk.push(c[3]);
    if (nh >= 3) stk.push(c[2]);
    if (nh >= 2) stk.push(c[1]);
    s.node = c[0];
    return nh > 0;
}

/* What both seed passes replay of a finished segment (rtcommon.h:411-466): the lights' skipped
   draws, 2 per light, and off the box at hp (normal hn) the cosine-hemisphere bounce, drawn even at
   the last depth */
__device__ __forceinline__ void light_draws(Seed &seed, uint32_t nl)
{
    for (uint32_t l = 0; l < nl; ++l) {
        (void)frand(seed);
        (void)frand(seed);
    }
}
__device__ __forceinline__ void box_bounce(Seed &seed, uint32_t nl, V3 hp, V3 hn, V3 &qo, V3 &qd)
{
    light_draws(seed, nl);
    const float r1 = frand(seed);
    const float r2 = frand(seed);
    const float ct = rt_sqrtf(1.0f - r1);
    const float st = rt_sqrtf(1.0f - ct * ct);
    const float phi = RT_M_2PI_F * r2;
    float sphi, cphi;
    rt_sincosf(phi, &sphi, &cphi);
    qd = shading_to_world(v3(cphi * st, sphi * st, ct), hn);
    qo = hp;
}

/* A seed pass's end of a sample, by the chain's writer lane: the sample's mesh-hit depth (0xff: only
   the box) of the chain's seeds at pslot ... */
__device__ __forceinline__ void seed_sample_end(const RtTriLaunch &a, uint32_t pslot, uint32_t sample, bool mesh_hit,
                                                uint32_t depth)
{
    if (a.split_hit_depth)
        a.split_hit_depth[(size_t)pslot * (a.sample_rate * a.sample_rate) + sample] =
            mesh_hit ? (uint8_t)depth : (uint8_t)0xffu;
}
/* ... and before the next sample the seed a chunk of split_fine samples starts from, or after the
   last the pixel's final seed and (true returned) its record of the RT_PIXEL_STATS diagnostics:
   its clocks, its steps, its camera rays that met the box, and `kind` */
__device__ __forceinline__ bool seed_sample_next(const RtTriLaunch &a, uint32_t pslot, uint32_t x, uint32_t yl,
                                                 uint32_t sample, Seed seed, uint32_t st_t0, uint32_t st_steps,
                                                 uint32_t st_box, uint32_t kind)
{
    const uint32_t spp = a.sample_rate * a.sample_rate;
    if (sample == spp || sample % a.split_fine == 0u) {
        const uint32_t c = sample == spp ? a.split_nseed - 1u : sample / a.split_fine;
        reinterpret_cast<uint2 *>(a.split_seed)[(size_t)pslot * a.split_nseed + c] = make_uint2(seed.x, seed.y);
    }
    if (sample != spp || !a.pixel_stats) return false;
    uint32_t *ps = pixel_stats_rec(a, x, yl);
    ps[0] = st_t0;
    ps[1] = (uint32_t)__builtin_amdgcn_s_memrealtime();
    ps[2] = st_steps;
    ps[3] = st_box;
    ps[4] = kind;
    return true;
}

template <int G> /* lanes per query: 1 (trav_step_q) or 4 (coop_round) */
__device__ __forceinline__ void seed_pass(const RtTriLaunch &a, int *s_stack)
{
    constexpr bool COOP = G > 1;
    Stack stk;
    stk.init(s_stack, a.spill, a.spill_cap);
    const int lane = (int)(threadIdx.x & 63), gbase = lane & ~(G - 1);
    CoopStack gst;
    gst.base = (lds_int *)(s_stack + (threadIdx.x & ~63u) + (uint32_t)gbase);
    if (COOP) /* the wave's stack words start as the root: an entry read before it is written is a node */
        for (int k = 0; k < RT_STACK_DEPTH; ++k) s_stack[k * RT_BLOCK + threadIdx.x] = 0;
    const float4 *__restrict__ nodes = reinterpret_cast<const float4 *>(a.nodes);
    const float4 *__restrict__ tris = reinterpret_cast<const float4 *>(a.tris);
    /* the root node (coop_root): a uniform address, so scalar loads */
    const uint4 *__restrict__ rootp = reinterpret_cast<const uint4 *>(a.nodes);
    const uint4 rq0 = rootp[0], rq1 = rootp[1], rq2 = rootp[2], rq3 = rootp[3];
    const uint32_t spp = a.sample_rate * a.sample_rate;
    const uint32_t tiles_x = (a.W + 7u) >> 3, tiles_y = (a.Hl + 7u) >> 3;
    const uint32_t n_items = a.split_which == RT_SPLIT_BOX ? box_items(a)
                                                           : tiles_x * tiles_y * 64u;
    const uint32_t nl = a.n_lights;
    const float hw = uniform_f(((float)a.W) / 2.0f);
    const float hh = uniform_f(((float)a.H) / 2.0f);
    const float bw = (float)RT_BOX_WIDTH, bh = (float)RT_BOX_HEIGHT;
    bool have = false, next = false, running = false, fin = false, drained = false;
    uint32_t x = 0, yl = 0, sample = 0, depth = 0;
    uint32_t pslot = 0; /* the chain's seeds: its pixel, or its slot (split_seed_slot) */
    uint32_t lpack = RT_LPACK_NONE; /* the pixel's candidate list (list_pack) */
    uint32_t bnext = 0, bend = 0; /* the wave's batch of queue items (batch_take) */
    Seed seed = {0u, 0u};
    V3 qo = v3(0.0f, 0.0f, 0.0f), qd = v3(0.0f, 0.0f, 1.0f);
    TravState ts = trav_idle();
    CoopQuery cq;
    coop_begin(cq, qo, qd, kInf);
    uint32_t st_steps = 0, st_box = 0, st_t0 = 0; /* diagnostics (RT_PIXEL_STATS): per pixel */
    uint32_t q_steps = 0;                          /* rounds of the current query */
    /* diagnostics builds (RT_SEED_STATS): per pixel the queries that took rounds, the queries
       answered in the path advance, and the loop iterations */
    uint32_t st_q = 0, st_imm = 0, st_it = 0;
    unsigned long long st_adv = 0, st_rnd = 0; /* clocks in the path advance / in stepping rounds */
    unsigned long long *const guard = a.counters + RT_CNT_GUARD; /* RT_GUARD_* flags (rt_synchronize) */
    for (;;) {
        /* lanes (COOP: groups) without a pixel take the next ones of the queue */
        /* takers: the first split_gpw lanes (COOP: 4-lane groups) of the wave */
        const uint32_t gpw = a.split_gpw ? a.split_gpw : 64u / G;
        const unsigned long long idle = __ballot(!have && lane == gbase && (uint32_t)(lane / G) < gpw);
        if (idle && !drained) {
            /* a batch per wave of as many items as it has takers */
            uint32_t item = batch_take(a.split_counter, idle, bnext, bend, gpw);
            if (COOP) item = __shfl(item, gbase);
            drained = bnext >= n_items;
            if (!have) {
                if (item < n_items) {
                    bool take;
                    if (a.split_which == RT_SPLIT_BOX) { /* the box pixels (long chains), by slot */
                        const uint32_t p = a.split_box[a.split_item_base + item];
                        x = p % a.W;
                        yl = p / a.W;
                        pslot = a.split_seed_slot ? item : p;
                        take = true;
                    } else {
                        take = tile_pixel(a, a.tile_order, item >> 6, item & 63u, tiles_x, x, yl);
                        if (take && a.split_which == RT_SPLIT_MESH) take = a.pixel_class[(size_t)yl * a.W + x] == -1;
                        pslot = yl * a.W + x;
                    }
                    if (take) {
                        seed = load_seed(a, seed_slot(a, x, yl));
                        lpack = list_pack(a, x, yl, tiles_x);
                        sample = 0;
                        have = true;
                        next = true;
                        if (a.pixel_stats) {
                            st_steps = st_box = 0;
                            if (RT_SEED_STATS) {
                                st_q = st_imm = st_it = 0;
                                st_adv = st_rnd = 0;
                            }
                            st_t0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
                        }
                    }
                }
            }
        }
        if (!__any(have)) {
            if (drained) break;
            continue;
        }
        /* The path advance, over as many segments and samples as it takes before the next stepping
           round: a new sample's camera ray, and every query answered without a round — an empty
           candidate list, a box bounce whose ray misses the root's child boxes (tested from
           registers) — advances at once, up to RT_SEED_IMM passes.  Box paths mostly
           leave the mesh's box alone, so a long chain's samples are mostly resolved here, without a
           memory round trip. */
        const unsigned long long t_adv0 = RT_SEED_STATS ? wave_clock() : 0ull;
        for (int pass = 0;; ++pass) {
            /* a new sample: the chunk's first seed, then the camera ray and its query */
            if (next) {
                next = false;
                if (lane == gbase &&
                    seed_sample_next(a, pslot, x, yl, sample, seed, st_t0, st_steps, st_box,
                                     1u + (uint32_t)a.split_which | (RT_SEED_STATS ? st_it << 4 : 0u)) &&
                    RT_SEED_STATS) {
                    uint32_t *ps = pixel_stats_rec(a, x, yl);
                    ps[7] = st_q << 16 | (st_imm & 0xffffu);
                    ps[5] = (uint32_t)(st_adv >> 6);
                    ps[6] = (uint32_t)(st_rnd >> 6);
                }
                if (sample == spp) {
                    have = false;
                } else {
                    camera_ray(a, seed, x, global_row(a, yl), sample / a.sample_rate, sample % a.sample_rate, hw, hh,
                               qo, qd);
                    depth = 0;
                    if (COOP) coop_begin(cq, qo, qd, kInf);
                    else trav_begin(ts, stk, qo, qd, kInf);
                    q_steps = 0;
                    running = true;
                    { /* the pixel's candidate list, as k_tris takes it */
                        if (lpack == RT_LPACK_EMPTY) {
                            running = false;
                            ts.best = -1;
                            cq.best = -1;
                            fin = true;
                        } else if (lpack != RT_LPACK_NONE) {
                            const ListRange lr = list_range(lpack);
                            if (COOP) { /* the group's stack, by its first lane (coop_round: the first block on top) */
                                const auto push = [&](int v) {
                                    if (lane == gbase) gst[cq.sp] = v;
                                    ++cq.sp;
                                };
                                push(list_leaves(lr.count, lr.first, push));
                            } else {
                                ts.node = list_leaves(lr.count, lr.first, [&](int v) { stk.push(v); });
                            }
                        } else if (COOP) { /* no list: the tree, from the root's children */
                            if (!coop_root(rq0, rq1, rq2, rq3, cq, gst, qd, lane == gbase)) {
                                running = false;
                                fin = true;
                            }
                        } else if (!lane_root(rq0, rq1, rq2, rq3, ts, stk, qd)) {
                            running = false;
                            fin = true;
                        }
                    }
                }
            }
            /* lanes whose query completed: the segment's draws, then the bounce or the next sample */
            if (fin) {
                fin = false;
                if (RT_SEED_STATS && q_steps == 0) ++st_imm; /* answered without a round */
                bool sample_done = true;
                const bool mesh_hit = (COOP ? cq.best : ts.best) >= 0;
                if (mesh_hit) { /* mesh hit: the light samples' draws, no bounce (rtcommon.h:411-421) */
                    light_draws(seed, nl);
                } else { /* the enclosing box (rtcommon.h:425-466) */
                    const float hd = intersect_box(qo, qd, RT_SMALL_F, bw, bh, bw);
                    if (depth == 0) ++st_box;
                    if (hd > RT_SMALL_F && hd < kInf) {
                        const V3 hp = v3(qo.x + qd.x * hd, qo.y + qd.y * hd, qo.z + qd.z * hd);
                        box_bounce(seed, nl, hp, box_normal(hp, bw, bh, bw), qo, qd);
                        ++depth;
                        if (depth <= a.max_depth) {
                            sample_done = false;
                            q_steps = 0;
                            running = true;
                            if (COOP) {
                                coop_begin(cq, qo, qd, kInf);
                                if (!coop_root(rq0, rq1, rq2, rq3, cq, gst, qd, lane == gbase)) {
                                    running = false; /* misses the mesh's box: no mesh hit, at once */
                                    fin = true;
                                }
                            } else {
                                trav_begin(ts, stk, qo, qd, kInf);
                                if (!lane_root(rq0, rq1, rq2, rq3, ts, stk, qd)) {
                                    running = false;
                                    fin = true;
                                }
                            }
                        }
                    }
                }
                if (sample_done) {
                    if (lane == gbase) seed_sample_end(a, pslot, sample, mesh_hit, depth);
                    ++sample;
                    next = true;
                }
            }
            /* at most RT_SEED_IMM passes before the next stepping round: the lanes whose queries
               need a traversal must not wait long for those whose answers come at once */
            if (pass + 1 >= RT_SEED_IMM || !__any(next || fin)) break;
        }
        unsigned long long t_rnd0 = 0;
        if (RT_SEED_STATS) {
            ++st_it;
            t_rnd0 = wave_clock();
            st_adv += t_rnd0 - t_adv0;
        }
        /* step the running queries (the box pixels' chains at top priority: they run beside the
           chunk tasks and set when the box pixels' chunks can start) */
        if (a.split_which == RT_SPLIT_BOX) __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int u = 0; u < RT_SEED_UNROLL; ++u) {
            if (running) {
                ++st_steps;
                ++q_steps;
                bool done;
                if constexpr (G == 4) {
                    done = coop_round(nodes, tris, cq, gst, qo, qd, RT_SMALL_F, a.n_nodes4, a.n_recs, a.coop_multi_sp,
                                      guard);
                } else {
                    TravCounts tc = {0u, 0u, 0u};
                    done = trav_step_q<false>(nodes, tris, ts, stk, qo, qd, RT_SMALL_F, false, tc);
                }
                /* The seed needs only WHETHER a segment hits the mesh (a hit ends the sample
                   after the light samples' draws, wherever it is): the query ends at its first
                   accepted triangle (the closest-hit rule's acceptance, t >= tmin) */
                const bool exists = (COOP ? cq.best : ts.best) >= 0; /* the query ends at its first accepted triangle */
                /* a query never takes 2^14 rounds (a ray meets far fewer nodes than that):
                   a bound every wave reaches, whatever a defect would do to a stack (reported) */
                if (q_steps > (1u << 14)) atomicOr(guard, (unsigned long long)RT_GUARD_ROUNDS);
                if (done || exists || q_steps > (1u << 14)) {
                    running = false;
                    fin = true;
                    if (RT_SEED_STATS) ++st_q;
                }
            }
        }
        if (RT_SEED_STATS) st_rnd += wave_clock() - t_rnd0;
    }
}

template <int G>
__global__ __launch_bounds__(RT_BLOCK, RT_TRIS_WAVES) void k_split_seeds(RtTriLaunch a)
{
    __shared__ int s_stack[RT_STACK_DEPTH * RT_BLOCK];
    seed_pass<G>(a, s_stack);
}

/* ------------------------------------------------------------------------ */
/* Subtree-parallel seed pass of the long chains (k_chain_seeds): G lanes per chain.  The seed
   needs only WHETHER a segment meets the mesh (an accepted triangle anywhere), and that answer
   is an OR over any cut of the tree: lane `sub` of a group owns edge `sub` of a fixed cut of the
   tree's top levels (a child slot of a node — chain_cut, breadth first, at most G edges), tests
   that child's box from an LDS copy of its parent's record when a query starts, and walks the
   subtree below alone, depth first, with k_tris's one-record step (trav_step_q) and its own
   stack; the query ends at the first step after which some lane of the group has accepted a
   triangle, or when every lane's subtree is exhausted.  A camera ray with a candidate list
   spreads the list's triangles over the lanes in runs of ceil(count / G).  The group's lanes
   carry the chain's path state alike (the same values computed in every lane), so a path
   advance costs one lane's instructions; the work of a query is split over G lanes without a
   shared stack or an item assignment (coop_round's cost: DESIGN.md §4.5). */
/* child slot k of a compressed node against the ray, unsorted: node_children's box test for one
   child (the same plane values: byte * 2^e * inv + (origin * inv - o * inv)) and the node's
   determinant cull.  Culling only. */
__device__ __forceinline__ bool edge_hit(uint4 q0, uint4 q1, uint4 q2, int k, V3 inv, V3 oi, V3 d)
{
    const uint32_t w = q0.w;
    const float sx = __builtin_amdgcn_ldexpf(inv.x, (int)(w & 31u) + RT_QEXP_MIN);
    const float sy = __builtin_amdgcn_ldexpf(inv.y, (int)((w >> 5) & 31u) + RT_QEXP_MIN);
    const float sz = __builtin_amdgcn_ldexpf(inv.z, (int)((w >> 10) & 31u) + RT_QEXP_MIN);
    const float bx = __builtin_fmaf(__uint_as_float(q0.x), inv.x, -oi.x);
    const float by = __builtin_fmaf(__uint_as_float(q0.y), inv.y, -oi.y);
    const float bz = __builtin_fmaf(__uint_as_float(q0.z), inv.z, -oi.z);
    const bool px = inv.x >= 0.0f, py = inv.y >= 0.0f, pz = inv.z >= 0.0f;
    const uint32_t sh = 8u * (uint32_t)k;
    const float nbx = (float)(((px ? q1.x : q1.y) >> sh) & 255u), fbx = (float)(((px ? q1.y : q1.x) >> sh) & 255u);
    const float nby = (float)(((py ? q1.z : q1.w) >> sh) & 255u), fby = (float)(((py ? q1.w : q1.z) >> sh) & 255u);
    const float nbz = (float)(((pz ? q2.x : q2.y) >> sh) & 255u), fbz = (float)(((pz ? q2.y : q2.x) >> sh) & 255u);
    const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(nbx, sx, bx), __builtin_fmaf(nby, sy, by)),
                                     __builtin_fmaxf(__builtin_fmaf(nbz, sz, bz), -1e-3f));
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaf(fbx, sx, bx), __builtin_fmaf(fby, sy, by)),
                                     __builtin_fmaf(fbz, sz, bz));
    if (!(tn <= tf)) return false;
    /* the determinant cull of node_children */
    const uint32_t nlo = q2.z, nhi = q2.w;
    const float nsc = __builtin_amdgcn_ldexpf(1.0f, (int)(nlo >> 24) - 128);
    const uint32_t sel_n = (px ? 4u : 0u) | (py ? 5u : 1u) << 8 | (pz ? 6u : 2u) << 16;
    const uint32_t sel_f = (px ? 0u : 4u) | (py ? 1u : 5u) << 8 | (pz ? 2u : 6u) << 16;
    const uint32_t nb = __builtin_amdgcn_perm(nhi, nlo, sel_n), fb = __builtin_amdgcn_perm(nhi, nlo, sel_f);
    const float bias = 128.0f * (d.x + d.y + d.z);
    const float fhi = __builtin_fmaf(d.x, (float)(nb & 0xffu),
                                     __builtin_fmaf(d.y, (float)((nb >> 8) & 0xffu),
                                                    __builtin_fmaf(d.z, (float)((nb >> 16) & 0xffu), -bias)));
    const float flo = __builtin_fmaf(d.x, (float)(fb & 0xffu),
                                     __builtin_fmaf(d.y, (float)((fb >> 8) & 0xffu),
                                                    __builtin_fmaf(d.z, (float)((fb >> 16) & 0xffu), -bias)));
    const float l1 = __builtin_fabsf(d.x) + __builtin_fabsf(d.y) + __builtin_fabsf(d.z);
    const float bound = __builtin_fmaf(__builtin_fmaxf(fhi, -flo) * nsc, 1.02f, 5e-7f * l1);
    return !(bound < 1e-4f);
}

__device__ __forceinline__ int link_of(uint4 l, int k) { return (int)(k == 0 ? l.x : k == 1 ? l.y : k == 2 ? l.z : l.w); }

/* The cut: the root's used child slots, then, level by level (a pass over the list in order), an
   edge to an inner node replaced by that node's used slots while the list stays within G edges.
   Thread 0 of the block, into s_par / s_slot; returns the edge count. */
template <int G>
__device__ int chain_cut(const uint4 *__restrict__ qn, uint32_t n_nodes, int *s_par, int *s_slot)
{
    if (n_nodes == 0) return 0;
    int n = 0;
    {
        const uint4 l = qn[3];
        for (int k = 0; k < 4; ++k)
            if (link_of(l, k) != RT_EMPTY_CHILD && n < G) {
                s_par[n] = 0;
                s_slot[n] = k;
                ++n;
            }
    }
    for (bool grew = true; grew;) {
        grew = false;
        for (int i = 0; i < n;) {
            const int c = link_of(qn[4 * s_par[i] + 3], s_slot[i]);
            if (c < 0 || c == RT_EMPTY_CHILD || (uint32_t)c >= n_nodes) {
                ++i;
                continue;
            }
            const uint4 l = qn[4 * c + 3];
            int m = 0;
            for (int k = 0; k < 4; ++k) m += link_of(l, k) != RT_EMPTY_CHILD ? 1 : 0;
            if (m == 0 || n - 1 + m > G) {
                ++i;
                continue;
            }
            for (int j = n - 1; j > i; --j) {
                s_par[j + m - 1] = s_par[j];
                s_slot[j + m - 1] = s_slot[j];
            }
            int t = i;
            for (int k = 0; k < 4; ++k)
                if (link_of(l, k) != RT_EMPTY_CHILD) {
                    s_par[t] = c;
                    s_slot[t] = k;
                    ++t;
                }
            n += m - 1;
            i += m; /* the new edges are the next level's: not expanded in this pass */
            grew = true;
        }
    }
    return n;
}

/* intersect_box (geometryFuncs.h:86-150) for a group of G >= 8 lanes carrying the same ray: the
   six slab divisions one per lane (lanes 0-5 of the group), gathered; the same operations on
   the same values as intersect_box, so the same bits. */
__device__ __forceinline__ float group_box(V3 o, V3 d, float tmin, float xs, float ys, float zs, int sub, int gbase)
{
    const int kk = sub < 6 ? sub : 0, ax = kk >> 1;
    const float oa = ax == 0 ? o.x : ax == 1 ? o.y : o.z, da = ax == 0 ? d.x : ax == 1 ? d.y : d.z;
    const float sa = ax == 0 ? xs : ax == 1 ? ys : zs;
    const float q = ((kk & 1) ? (0.0f + sa) - oa : (0.0f - sa) - oa) / da;
    const float tx1 = __shfl(q, gbase), tx2 = __shfl(q, gbase + 1), ty1 = __shfl(q, gbase + 2);
    const float ty2 = __shfl(q, gbase + 3), tz1 = __shfl(q, gbase + 4), tz2 = __shfl(q, gbase + 5);
    float nt = 0.0f, ft = rt_inff();
    if (d.x != 0) {
        nt = rt_minf(tx1, tx2);
        ft = rt_maxf(tx1, tx2);
    } else if (rt_fabsf(o.x - 0.0f) > xs) {
        return 0;
    }
    if (d.y != 0) {
        if (ty1 > ty2) {
            nt = rt_maxf(ty2, nt);
            ft = rt_minf(ty1, ft);
        } else {
            nt = rt_maxf(ty1, nt);
            ft = rt_minf(ty2, ft);
        }
    } else if (rt_fabsf(o.y - 0.0f) > ys) {
        return 0;
    }
    if (d.z != 0) {
        if (tz1 > tz2) {
            nt = rt_maxf(tz2, nt);
            ft = rt_minf(tz1, ft);
        } else {
            nt = rt_maxf(tz1, nt);
            ft = rt_minf(tz2, ft);
        }
    } else if (rt_fabsf(o.z - 0.0f) > zs) {
        return 0;
    }
    if (nt > ft || ft < tmin) return rt_inff();
    if (nt < tmin) return ft;
    return nt;
}

/* box_normal (geometryFuncs.h:71-84): -p / |p| is exactly -1 or +1 for a finite non-zero p, so the
   division runs only for the rest (0 or infinite: NaN, as the reference's) */
__device__ __forceinline__ float neg_sign(float p)
{
    if (p != 0.0f && rt_fabsf(p) < rt_inff()) return p > 0.0f ? -1.0f : 1.0f;
    return -p / rt_fabsf(p);
}
__device__ __forceinline__ V3 box_normal_signs(V3 p, float xs, float ys, float zs)
{
    const float dx = rt_fabsf(rt_fabsf(p.x) - xs);
    const float dy = rt_fabsf(rt_fabsf(p.y) - ys);
    const float dz = rt_fabsf(rt_fabsf(p.z) - zs);
    if (dx < dy && dx < dz) return v3(neg_sign(p.x), 0.0f, 0.0f);
    if (dy < dz) return v3(0.0f, neg_sign(p.y), 0.0f);
    return v3(0.0f, 0.0f, neg_sign(p.z));
}

/* camera_dir for a group of G >= 8 lanes: the three divisions by the length on lanes 0-2 */
__device__ __forceinline__ V3 group_camera_dir(const rt_camera &cam, float a, float b, int sub, int gbase)
{
    const float x = (cam.view.x + cam.right.x * a) + cam.up.x * b;
    const float y = (cam.view.y + cam.right.y * a) + cam.up.y * b;
    const float z = (cam.view.z + cam.right.z * a) + cam.up.z * b;
    const float w = (cam.view.w + cam.right.w * a) + cam.up.w * b;
    const float len = rt_sqrtf(((x * x + y * y) + z * z) + w * w);
    const int kk = sub < 3 ? sub : 0;
    const float q = (kk == 0 ? x : kk == 1 ? y : z) / len;
    return v3(__shfl(q, gbase), __shfl(q, gbase + 1), __shfl(q, gbase + 2));
}

template <int G, bool RUNS = false> /* RUNS: the repair pass's runs of hit samples */
__global__ __launch_bounds__(RT_BLOCK, RT_TRIS_WAVES) void k_chain_seeds(RtTriLaunch a)
{
    static_assert(G >= 8 && G <= 64 && (G & (G - 1)) == 0, "the advance spreads 6 divisions over the group's lanes");
    __shared__ int s_stack[RT_STACK_DEPTH * RT_BLOCK];
    __shared__ uint4 s_erec[G][4]; /* per edge: its parent's record */
    __shared__ int s_par[G], s_slot[G];
    __shared__ int s_ne;
    if (box_items(a) == 0u) return; /* an empty list (the repair pass, mostly): no cut to make */
    const uint4 *__restrict__ qn = reinterpret_cast<const uint4 *>(a.nodes);
    if (threadIdx.x == 0) s_ne = chain_cut<G>(qn, a.n_nodes4, s_par, s_slot);
    __syncthreads();
    const int ne = s_ne;
    for (int i = (int)threadIdx.x; i < 4 * ne; i += RT_BLOCK) s_erec[i >> 2][i & 3] = qn[4 * s_par[i >> 2] + (i & 3)];
    __syncthreads();
    __builtin_amdgcn_s_setprio(3); /* the long chains run beside the chunk tasks and set when their own chunks start */

    Stack stk;
    stk.init(s_stack, a.spill, a.spill_cap);
    const int lane = (int)(threadIdx.x & 63), sub = lane & (G - 1), gbase = lane & ~(G - 1);
    const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << gbase;
    const float4 *__restrict__ nodes = reinterpret_cast<const float4 *>(a.nodes);
    const float4 *__restrict__ tris = reinterpret_cast<const float4 *>(a.tris);
    const int eslot = sub < ne ? s_slot[sub] : 0;
    const uint32_t spp = a.sample_rate * a.sample_rate, fine = a.split_fine, nseed = a.split_nseed;
    const uint32_t tiles_x = (a.W + 7u) >> 3;
    const uint32_t n_items = box_items(a);
    const uint32_t nl = a.n_lights;
    const float hw = uniform_f(((float)a.W) / 2.0f);
    const float hh = uniform_f(((float)a.H) / 2.0f);
    const float bw = (float)RT_BOX_WIDTH, bh = (float)RT_BOX_HEIGHT;
    const uint32_t gpw = a.split_gpw ? a.split_gpw : 64u / G;
    bool have = false, next = false, running = false, fin = false, drained = false, live = false, ghit = false;
    uint32_t x = 0, yl = 0, sample = 0, depth = 0, pslot = 0; /* pslot: the chain's seeds (pixel or slot) */
    uint32_t lpack = RT_LPACK_NONE;
    uint32_t bnext = 0, bend = 0;
    Seed seed = {0u, 0u};
    V3 qo = v3(0.0f, 0.0f, 0.0f), qd = v3(0.0f, 0.0f, 1.0f);
    TravState ts = trav_idle();
    uint32_t st_steps = 0, st_box = 0, st_t0 = 0, q_steps = 0;
    unsigned long long *const guard = a.counters + RT_CNT_GUARD;
    /* a query of the tree starts at the lane's edge of the cut; false: no lane of the group
       enters its child's box (no mesh hit, without a step) */
    auto start_tree = [&]() -> bool {
        live = false;
        if (sub < ne) {
            const uint4 p0 = s_erec[sub][0], p1 = s_erec[sub][1], p2 = s_erec[sub][2], p3 = s_erec[sub][3];
            if (edge_hit(p0, p1, p2, eslot, ts.inv, ts.oi, qd)) {
                live = true;
                ts.node = link_of(p3, eslot);
            }
        }
        return (__ballot(live) & gmask) != 0ull;
    };
    for (;;) {
        const unsigned long long idle = __ballot(!have && lane == gbase && (uint32_t)(lane / G) < gpw);
        if (idle && !drained) {
            uint32_t item = batch_take(a.split_counter, idle, bnext, bend, gpw);
            item = __shfl(item, gbase);
            drained = bnext >= n_items;
            if (!have && item < n_items) {
                const uint32_t p = a.split_box[a.split_item_base + item];
                pslot = a.split_seed_slot ? item : p;
                x = p % a.W;
                yl = p / a.W;
                seed = load_seed(a, seed_slot(a, x, yl));
                sample = 0;
                if (a.split_restart) { /* a repaired pixel: from its first missed chunk, whose seed the
                                          jump gives (every sample before it hit the mesh) */
                    const uint32_t ch = a.split_restart[p];
                    const uint32_t k = ch * a.split_restart_chunk * a.split_spec_draws;
                    seed.x = mwc_jump<36969u>(seed.x, k, a.split_spec_mul[2 * ch]);
                    seed.y = mwc_jump<18000u>(seed.y, k, a.split_spec_mul[2 * ch + 1]);
                    sample = ch * a.split_restart_chunk;
                }
                lpack = list_pack(a, x, yl, tiles_x);
                have = true;
                next = true;
                if (a.pixel_stats) {
                    st_steps = st_box = 0;
                    st_t0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
                }
            }
        }
        if (!__any(have)) {
            if (drained) break;
            continue;
        }
        /* the path advance (alike in the group's lanes), up to RT_CHAIN_IMM passes: a finished
           query's bounce (or the end of its sample), a new sample's camera ray, then at most one
           query start per pass — its ray answered at once when it enters no subtree's box.  The
           advance's IEEE divisions are spread over the group's lanes (one each, gathered) */
        for (int pass = 0;; ++pass) {
            bool start = false;
            if (fin) {
                fin = false;
                bool sample_done = true;
                if (ghit) { /* mesh hit: the light samples' draws, no bounce (rtcommon.h:411-421) */
                    light_draws(seed, nl);
                } else { /* the enclosing box (rtcommon.h:425-466) */
                    const float hd = group_box(qo, qd, RT_SMALL_F, bw, bh, bw, sub, gbase);
                    if (depth == 0) ++st_box;
                    if (hd > RT_SMALL_F && hd < kInf) {
                        const V3 hp = v3(qo.x + qd.x * hd, qo.y + qd.y * hd, qo.z + qd.z * hd);
                        box_bounce(seed, nl, hp, box_normal_signs(hp, bw, bh, bw), qo, qd);
                        ++depth;
                        if (depth <= a.max_depth) {
                            sample_done = false;
                            start = true;
                        }
                    }
                }
                if (sample_done) {
                    /* (not the repair pass: split_hit_depth is NULL there) */
                    if (!RUNS && lane == gbase) seed_sample_end(a, pslot, sample, ghit, depth);
                    ++sample;
                    next = true;
                }
            }
            bool run_on = false;
            if (RUNS && next && a.split_restart && sample < spp && lpack != RT_LPACK_NONE &&
                lpack != RT_LPACK_EMPTY) {
                /* the repair pass (a speculated pixel's chain): a run of up to G - 1 samples at once,
                   one per lane, each from the seed it has if every earlier sample of the run hit the
                   mesh (split_spec_draws numbers each, rtcommon.h:411-421), its camera ray tested
                   against the pixel's candidate list; the chain takes the run up to its first miss */
                const uint32_t D = a.split_spec_draws, rem = spp - sample;
                const uint32_t runmax = rem < (uint32_t)(G - 1) ? rem : (uint32_t)(G - 1);
                /* frand's state stepped sub x D draws on (rng.h:24-42): one multiplication by the
                   jump multiplier of the lane (mwc_jump) */
                Seed sl;
                sl.x = mwc_jump<36969u>(seed.x, (uint32_t)sub * D, a.split_run_mul[2 * sub]);
                sl.y = mwc_jump<18000u>(seed.y, (uint32_t)sub * D, a.split_run_mul[2 * sub + 1]);
                bool hit = false;
                if ((uint32_t)sub < runmax) {
                    const uint32_t s = sample + (uint32_t)sub;
                    Seed sc = sl;
                    V3 o, dd;
                    camera_ray(a, sc, x, global_row(a, yl), s / a.sample_rate, s % a.sample_rate, hw, hh, o, dd);
                    const ListRange lr = list_range(lpack);
                    for (uint32_t t = 0; t < lr.count && !hit; ++t) {
                        const uint32_t r = lr.first + t;
                        float tt = 0.0f;
                        const bool h = mt_test(o, dd, tris[3 * r], tris[3 * r + 1], tris[3 * r + 2], tt);
                        hit = h && !(tt < RT_SMALL_F) && tt <= kInf; /* the closest-hit acceptance */
                    }
                }
                /* the run's hits before its first miss (64-bit: a group may be the whole wave; lane
                   runmax <= G - 1 never hits, so ~hm has a set bit) */
                const unsigned long long hm = (__ballot(hit) & gmask) >> gbase;
                uint32_t m = (uint32_t)__builtin_ctzll(~hm);
                if (m > runmax) { /* a defect: reported (rt_synchronize fails the render), the run taken as ended */
                    if (lane == gbase) atomicOr(guard, (unsigned long long)RT_GUARD_INDEX);
                    m = runmax;
                }
                if ((uint32_t)sub < m && (sample + (uint32_t)sub) % fine == 0u)
                    reinterpret_cast<uint2 *>(a.split_seed)[(size_t)pslot * nseed + (sample + (uint32_t)sub) / fine] =
                        make_uint2(sl.x, sl.y);
                seed.x = (uint32_t)__shfl((int)sl.x, gbase + (int)m);
                seed.y = (uint32_t)__shfl((int)sl.y, gbase + (int)m);
                sample += m;
                /* a whole run of hits: the next run in the next pass; else the missed sample (or the
                   chain's end) goes on below */
                run_on = m == runmax && sample < spp;
            }
            if (next && !run_on) {
                next = false;
                if (lane == gbase)
                    (void)seed_sample_next(a, pslot, x, yl, sample, seed, st_t0, st_steps, st_box,
                                           1u + (uint32_t)RT_SPLIT_BOX);
                if (sample == spp) {
                    have = false;
                } else {
                    /* strat_rand twice (rng.h:45-47): the two draws, then the divisions on two lanes */
                    const float f1 = frand(seed), f2 = frand(seed);
                    const uint32_t sx = sample / a.sample_rate, sy = sample % a.sample_rate;
                    const float num = (float)(sub & 1 ? sy : sx) + (sub & 1 ? f2 : f1);
                    const float qv = num / (float)a.sample_rate;
                    const float ua = __shfl(qv, gbase), ub = __shfl(qv, gbase + 1);
                    const float fa = (float)x + ua;
                    const uint32_t y = global_row(a, yl);
                    const float fb = (float)y + ub;
                    qo = v3(a.cam.position.x, a.cam.position.y, a.cam.position.z);
                    qd = group_camera_dir(a.cam, fa - hw, fb - hh, sub, gbase);
                    depth = 0;
                    start = true;
                }
            }
            if (start) {
                trav_begin(ts, stk, qo, qd, kInf);
                q_steps = 0;
                running = true;
                if (depth == 0 && lpack == RT_LPACK_EMPTY) { /* no candidate: no mesh hit */
                    running = false;
                    ghit = false;
                    fin = true;
                } else if (depth == 0 && lpack != RT_LPACK_NONE) { /* the list's triangles in runs over the lanes */
                    const ListRange lr = list_range(lpack);
                    const uint32_t bs = (lr.count + (uint32_t)G - 1u) / (uint32_t)G, s0 = (uint32_t)sub * bs;
                    live = s0 < lr.count;
                    const uint32_t cnt = live ? (lr.count - s0 < bs ? lr.count - s0 : bs) : 1u;
                    ts.node = ~(int)(((lr.first + s0) << 3) | (cnt - 1u));
                } else if (!start_tree()) { /* misses every subtree's box: no mesh hit, at once */
                    running = false;
                    ghit = false;
                    fin = true;
                }
            }
            if (pass + 1 >= RT_CHAIN_IMM || !__any(next || fin)) break;
        }
        /* traversal steps: each live lane one record of its subtree; the group's query ends at
           its first accepted triangle or when no lane has a subtree left */
#pragma unroll
        for (int u = 0; u < RT_CHAIN_UNROLL; ++u) {
            bool found = false;
            if (running && live) {
                const int nd = ts.node;
                const uint32_t enc = ~(uint32_t)nd;
                const bool bad = nd < 0 ? (enc >> 3) + (enc & 7u) >= a.n_recs : (uint32_t)nd >= a.n_nodes4;
                if (bad) { /* a defect: reported (rt_synchronize fails the render), the lane ends */
                    atomicOr(guard, (unsigned long long)RT_GUARD_INDEX);
                    live = false;
                } else {
                    TravCounts tc = {0u, 0u, 0u};
                    const bool done = trav_step_q<false>(nodes, tris, ts, stk, qo, qd, RT_SMALL_F, false, tc);
                    found = ts.best >= 0;
                    if (done) live = false;
                }
            }
            const unsigned long long fb = __ballot(found), lb = __ballot(live);
            if (running) {
                ++q_steps;
                ++st_steps;
                const bool gf = (fb & gmask) != 0ull, gl = (lb & gmask) != 0ull;
                /* a query never takes 2^14 steps: a bound every wave reaches (reported) */
                if (q_steps > (1u << 14) && lane == gbase) atomicOr(guard, (unsigned long long)RT_GUARD_ROUNDS);
                if (gf || !gl || q_steps > (1u << 14)) {
                    running = false;
                    live = false;
                    fin = true;
                    ghit = gf;
                }
            }
        }
    }
}

/* Sample-split tiles, step 3 (per part: the long chains after their chunks on the second stream,
   the clean mesh pixels after theirs on a third, the repaired after the repair pass): per pixel,
   the samples' radiance summed in sample order
   (raytracer.cl:228-230: the same additions on the same values as one lane's loop), the
   pixel written (:234-240) and its final seed (:241-242). */
__global__ __launch_bounds__(RT_BLOCK) void k_split_finish(RtTriLaunch a)
{
    const uint32_t npx = a.W * a.Hl;
    /* every pixel, or the clean mesh pixels (RT_FIN_MESH), over a grid-stride loop */
    const uint32_t n = npx;
    for (uint32_t i = blockIdx.x * RT_BLOCK + threadIdx.x; i < n; i += gridDim.x * RT_BLOCK) {
        const uint32_t p = i;
        if (p >= npx) continue;
        if (a.finish_part == RT_FIN_MESH && (a.pixel_class[p] >= 0 || (a.split_dirty && a.split_dirty[p] != ~0u)))
            continue; /* the mesh pixels no chunk of which missed */
        const uint32_t spp = a.sample_rate * a.sample_rate;
        float acc_x = 0.0f, acc_y = 0.0f, acc_z = 0.0f;
        /* 16 samples' loads issued together, then added in sample order (a part's few pixels are
           latency-bound: one load per add would wait out each) */
        for (uint32_t s0 = 0; s0 < spp; s0 += 16u) {
            float v[48];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t s = s0 + (uint32_t)j < spp ? s0 + (uint32_t)j : spp - 1u;
                const float *c = a.split_col + ((size_t)s * npx + p) * 3u;
                v[3 * j] = c[0];
                v[3 * j + 1] = c[1];
                v[3 * j + 2] = c[2];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (s0 + (uint32_t)j < spp) {
                    acc_x += v[3 * j];
                    acc_y += v[3 * j + 1];
                    acc_z += v[3 * j + 2];
                }
            }
        }
        write_pixel(reinterpret_cast<float4 *>(a.out) + p, pixel_mean(acc_x, acc_y, acc_z, (float)spp),
                    a.progressive > 0, 1.0f / (float)a.progressive);
        const uint32_t x = p % a.W, yl = p / a.W;
        const uint32_t slot = seed_slot(a, x, yl);
        const uint2 sd = reinterpret_cast<const uint2 *>(a.split_seed)[(size_t)p * a.split_nseed + a.split_nseed - 1u];
        store_seed(a, slot, sd.x, sd.y);
    }
}

/* The in-order sums of a part's listed pixels (the long chains, the repaired): a wave per pixel —
   its lanes load the samples together (4 each per 256), then the wave adds them in sample order
   through readlane, the same additions as k_split_finish's loop.  A part is a few thousand pixels
   at most, latency-bound when one lane walks a pixel's samples. */
__global__ __launch_bounds__(RT_BLOCK) void k_split_finish_list(RtTriLaunch a)
{
    const uint32_t npx = a.W * a.Hl, lane = threadIdx.x & 63u;
    const uint32_t n = box_items(a);
    const uint32_t spp = a.sample_rate * a.sample_rate;
    for (uint32_t i = blockIdx.x * (RT_BLOCK / 64u) + (threadIdx.x >> 6); i < n; i += gridDim.x * (RT_BLOCK / 64u)) {
        const uint32_t p = a.split_box[a.split_item_base + i];
        if (p >= npx) continue;
        float acc_x = 0.0f, acc_y = 0.0f, acc_z = 0.0f;
        for (uint32_t b = 0; b < spp; b += 256u) {
            float v[12];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t s = b + lane * 4u + (uint32_t)j;
                const float *c = a.split_col + ((size_t)(s < spp ? s : 0u) * npx + p) * 3u;
                v[3 * j] = c[0];
                v[3 * j + 1] = c[1];
                v[3 * j + 2] = c[2];
            }
            const uint32_t lanes = (spp - b + 3u) / 4u < 64u ? (spp - b + 3u) / 4u : 64u;
            for (uint32_t l = 0; l < lanes; ++l) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (b + l * 4u + (uint32_t)j < spp) {
                        acc_x += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[3 * j]), (int)l));
                        acc_y += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[3 * j + 1]), (int)l));
                        acc_z += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[3 * j + 2]), (int)l));
                    }
                }
            }
        }
        if (lane != 0u) continue;
        write_pixel(reinterpret_cast<float4 *>(a.out) + p, pixel_mean(acc_x, acc_y, acc_z, (float)spp),
                    a.progressive > 0, 1.0f / (float)a.progressive);
        const uint32_t x = p % a.W, yl = p / a.W;
        const uint32_t slot = seed_slot(a, x, yl);
        const uint2 sd = reinterpret_cast<const uint2 *>(
            a.split_seed)[(size_t)(a.split_seed_slot ? i : p) * a.split_nseed + a.split_nseed - 1u];
        store_seed(a, slot, sd.x, sd.y);
    }
}

} // namespace

int rt_launch_split_seeds(const RtTriLaunch &a, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(a.split_counter, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return (int)e;
    const dim3 g(a.split_seed_blocks), b(RT_BLOCK);
    if (a.split_which == RT_SPLIT_BOX && a.split_coop >= 8) { /* subtree-parallel */
        if (a.split_coop == 64 && a.split_restart) hipLaunchKernelGGL((k_chain_seeds<64, true>), g, b, 0, st, a);
        else if (a.split_coop == 32 && a.split_restart) hipLaunchKernelGGL((k_chain_seeds<32, true>), g, b, 0, st, a);
        else if (a.split_coop == 16 && a.split_restart) hipLaunchKernelGGL((k_chain_seeds<16, true>), g, b, 0, st, a);
        else if (a.split_coop == 8 && a.split_restart) hipLaunchKernelGGL((k_chain_seeds<8, true>), g, b, 0, st, a);
        else if (a.split_coop == 8) hipLaunchKernelGGL(k_chain_seeds<8>, g, b, 0, st, a);
        else if (a.split_coop == 32) hipLaunchKernelGGL(k_chain_seeds<32>, g, b, 0, st, a);
        else if (a.split_coop == 64) hipLaunchKernelGGL(k_chain_seeds<64>, g, b, 0, st, a);
        else hipLaunchKernelGGL(k_chain_seeds<16>, g, b, 0, st, a);
    } else if (a.split_coop == RT_SEED_COOP4) hipLaunchKernelGGL(k_split_seeds<4>, g, b, 0, st, a);
    else hipLaunchKernelGGL(k_split_seeds<1>, g, b, 0, st, a);
    return (int)hipGetLastError();
}

int rt_launch_split_finish(const RtTriLaunch &a, void *stream)
{
    if (a.finish_part == RT_FIN_LIST) { /* a wave per listed pixel */
        const uint32_t n = a.split_n_dev ? 4096u : a.split_n_box; /* a count on the device: grid-stride */
        const uint32_t blocks = std::min(2048u, std::max(1u, (n + 3u) / 4u));
        hipLaunchKernelGGL(k_split_finish_list, dim3(blocks), dim3(RT_BLOCK), 0, (hipStream_t)stream, a);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(k_split_finish, dim3((a.W * a.Hl + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
