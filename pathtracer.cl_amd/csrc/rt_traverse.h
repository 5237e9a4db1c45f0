/*
 * rt_traverse.h — the per-lane ray queries of the gfx950 kernels: the reference's
 * ray/triangle test, the LDS traversal stack with its global spill tail, and the
 * resumable traversal of the 4-wide trees (full-precision and compressed nodes) with
 * the linear loop beside them; a query's idle state (trav_idle) and a candidate list as
 * the traversal's virtual leaves (list_leaves).  Shared by rt_tris.hip and rt_split.hip (the render
 * kernels), rt_spheres.hip (the batch ray queries), rt_sched.hip (the cost probe),
 * rt_lists.hip and rt_features.hip (the first-hit feature kernel); everything here has
 * internal linkage.
 */
#ifndef RT_TRAVERSE_H
#define RT_TRAVERSE_H

#include <hip/hip_runtime.h>

#include "rt_device.h"
#include "rt_internal.h"
#include "rt_quant.h"

#pragma clang fp contract(off)

namespace {

constexpr float kInf = __builtin_huge_valf();

/* ------------------------------------------------------------------------ */
/* Ray/triangle test (geometryFuncs.h:160-245): barycentric part shared by the
   closest-hit and any-hit forms.  Returns false on rejection, else t.        */
__device__ __forceinline__ bool mt_test(V3 o, V3 d, const float4 &a, const float4 &b, const float4 &c, float &t)
{
    const V3 v0 = v3(a.x, a.y, a.z);
    const V3 e1 = v3(b.x, b.y, b.z);
    const V3 e2 = v3(c.x, c.y, c.z);
    const V3 p = cross3(d, e2);
    const float det = dot3(p, e1);
    /* Evaluated without early exits so that the vertex fetch is not sunk below the
       determinant test; the accepted path computes exactly the reference's values. */
    const float inv = 1.0f / det;
    const V3 to = v3(o.x - v0.x, o.y - v0.y, o.z - v0.z);
    const V3 q = cross3(to, e1);
    const float u = dot3(p, to) * inv;
    const float v = dot3(q, d) * inv;
    t = dot3(q, e2) * inv;
    return !(rt_fabsf(det) < RT_SMALL_F) && !(u < 0 || u > 1) && !(v < 0 || v + u > 1);
}

/* Conservative slab test against one child box (culling only: no parity
   constraint, explicit FMAs allowed). */
__device__ __forceinline__ float slab(float lo_x, float hi_x, float lo_y, float hi_y, float lo_z, float hi_z, V3 inv,
                                      V3 oi, float tmin_c, float tmax_c, bool &hit)
{
    const float x0 = __builtin_fmaf(lo_x, inv.x, -oi.x);
    const float x1 = __builtin_fmaf(hi_x, inv.x, -oi.x);
    const float y0 = __builtin_fmaf(lo_y, inv.y, -oi.y);
    const float y1 = __builtin_fmaf(hi_y, inv.y, -oi.y);
    const float z0 = __builtin_fmaf(lo_z, inv.z, -oi.z);
    const float z1 = __builtin_fmaf(hi_z, inv.z, -oi.z);
    const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(x0, x1), __builtin_fminf(y0, y1)),
                                     __builtin_fmaxf(__builtin_fminf(z0, z1), tmin_c));
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(x0, x1), __builtin_fmaxf(y0, y1)),
                                     __builtin_fminf(__builtin_fmaxf(z0, z1), tmax_c));
    hit = tn <= tf;
    return tn;
}

__device__ __forceinline__ float safe_rcp(float d)
{
    const float e = 1e-18f;
    const float dd = (rt_fabsf(d) > e) ? d : (d < 0.0f ? -e : e);
    return __builtin_amdgcn_rcpf(dd);
}

/* Culling margin on the t interval: covers the rounding of the reference's
   intersection t relative to the box slabs (boxes are padded as well). */
__device__ __forceinline__ float t_slack(float t) { return t * 1.0009765625f + 1e-4f; }

struct TravCounts {
    uint32_t nodes;
    uint32_t tests;
    uint32_t leaves;
};

/* Leaf of the full-precision traversals (trav_step, traverse): the reference's triangle tests on
   slots [first, first+count), in order, ending at an any-hit query's first occluder. */
template <bool COUNT>
__device__ __forceinline__ bool leaf_accept(int s, float4 a, V3 d, bool ok, float t, float tmin, float tmax,
                                            bool any_hit, int &best, int &best_orig, float &best_t, bool &done)
{
    if (!ok) return false;
    if (any_hit) {
        if (t < tmax && t > tmin) {
            best = s;
            done = true;
        }
    } else {
        const int orig = __float_as_int(a.w);
        if (!(t < tmin) && (t < best_t || (t == best_t && orig > best_orig))) {
            best = s;
            best_orig = orig;
            best_t = t;
            return true;
        }
    }
    return false;
}

template <bool COUNT>
__device__ __forceinline__ bool leaf_tests(const float4 *__restrict__ tris, int first, int count, V3 o, V3 d,
                                           float tmin, float tmax, bool any_hit, int &best, int &best_orig,
                                           float &best_t, TravCounts &cnt)
{
    bool done = false;
    for (int k = 0; k < count; ++k) {
        const int s0 = first + k;
        const float4 a0 = tris[3 * s0], b0 = tris[3 * s0 + 1], c0 = tris[3 * s0 + 2];
        if (COUNT) cnt.tests++;
        float t0 = 0.0f;
        const bool h0 = mt_test(o, d, a0, b0, c0, t0);
        leaf_accept<COUNT>(s0, a0, d, h0, t0, tmin, tmax, any_hit, best, best_orig, best_t, done);
        if (done) return true;
    }
    return false;
}

/* Per-lane traversal stack: [depth][lane] in LDS (stride RT_BLOCK dwords, bank
   conflict free) with an overflow tail in global memory for the rare rays of a
   4-wide tree whose worst-case stack exceeds RT_STACK_DEPTH.  The two parts are
   typed by address space, so that a pop that may come from either stays a
   ds_read plus a global load under lane masks — never a generic (flat) load, which
   would occupy the vector-memory address path for every LDS pop. */
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) int lds_int;
typedef __attribute__((address_space(3))) float lds_float;
typedef __attribute__((address_space(1))) int32_t glob_int;
#else
typedef int lds_int;
typedef float lds_float;
typedef int32_t glob_int;
#endif

struct Stack {
    lds_int *lds;
    glob_int *spill_block; /* the block's spill area (uniform): lane l owns [l * cap, (l + 1) * cap) */
    uint32_t cap;
    int sp;
    __device__ __forceinline__ glob_int *spill_slot(int i) const
    {
        return spill_block + threadIdx.x * cap + (uint32_t)(i - RT_STACK_DEPTH);
    }
    __device__ __forceinline__ void push(int v)
    {
        if (sp < RT_STACK_DEPTH) lds[sp * RT_BLOCK] = v;
        else *spill_slot(sp) = v;
        ++sp;
    }
    __device__ __forceinline__ int pop()
    {
        --sp;
        int v;
        if (sp < RT_STACK_DEPTH) v = lds[sp * RT_BLOCK];
        else v = *spill_slot(sp);
        return v;
    }
    __device__ __forceinline__ void init(int *lds_base, int32_t *spill_base, uint32_t spill_cap)
    {
        lds = (lds_int *)(lds_base + threadIdx.x);
        spill_block = (glob_int *)(spill_base + (size_t)blockIdx.x * RT_BLOCK * spill_cap);
        cap = spill_cap;
        sp = 0;
    }
};

__device__ __forceinline__ void cas(float &ta, int &ca, float &tb, int &cb)
{
    const bool sw = tb < ta;
    const float t = sw ? tb : ta;
    const int c = sw ? cb : ca;
    tb = sw ? ta : tb;
    cb = sw ? ca : cb;
    ta = t;
    ca = c;
}

/* Resumable per-lane traversal of the binary or 4-wide tree: the whole query
   state is this struct plus the lane's stack, so a query can be advanced one
   node (or one leaf) at a time and suspended between steps. */
struct TravState {
    int node;      /* next node to visit (>= 0 inner, < 0 leaf) */
    int best;      /* leaf-order slot of the current closest / occluding hit, -1 none */
    int best_orig; /* its original triangle index (tie rule) */
    float best_t;  /* closest hit so far (= tmax of an any-hit query) */
    V3 inv, oi;    /* 1/d and o/d for the slab tests */
};

__device__ __forceinline__ void trav_begin(TravState &s, Stack &stk, V3 o, V3 d, float tmax)
{
    s.inv = v3(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
    s.oi = v3(o.x * s.inv.x, o.y * s.inv.y, o.z * s.inv.z);
    s.node = 0;
    s.best = -1;
    s.best_orig = -1;
    s.best_t = tmax;
    stk.sp = 0;
}

/* the state of a lane without a query */
__device__ __forceinline__ TravState trav_idle()
{
    TravState s;
    s.node = 0;
    s.best = -1;
    s.best_orig = -1;
    s.best_t = kInf;
    s.inv = v3(0.0f, 0.0f, 0.0f);
    s.oi = s.inv;
    return s;
}

/* A candidate list (`count` records from slot `first`, a multiple of 8: rt_kernel_util.h
   list_range) as virtual leaves of at most 8 records: the later blocks pushed, last first, the
   first block returned — a per-lane query's cursor, a cooperative one's top entry. */
template <class Push>
__device__ __forceinline__ int list_leaves(uint32_t count, uint32_t first, Push push)
{
    for (uint32_t b = (count - 1u) >> 3; b > 0u; --b) {
        const uint32_t k = count - 8u * b < 8u ? count - 8u * b : 8u;
        push(~(int)(((first + 8u * b) << 3) | (k - 1u)));
    }
    return ~(int)((first << 3) | ((count < 8u ? count : 8u) - 1u));
}

/* Half `hi` of a word of two f16 values, widened to f32 (exact; folds into the
   op_sel of v_fma_mix_f32). */
__device__ __forceinline__ float half_of(uint32_t w, int hi)
{
    const uint16_t b = (uint16_t)(hi ? (w >> 16) : (w & 0xffffu));
    return (float)__builtin_bit_cast(_Float16, b);
}

/* The 4 child boxes of a compressed node (rt_quant.h; the record as its four dwordx4 words)
   against the ray: c[] the children by their sort key t[] ascending (misses last, kInf); returns
   how many were hit (0 also when the determinant cull skips the subtree).  Culling only. */
__device__ __forceinline__ int node_children(uint4 q0, uint4 q1, uint4 q2, uint4 q3, V3 inv, V3 oi, V3 d,
                                         float best_t, bool any_hit, bool longest, float (&t)[4], int (&c)[4])
{
    const float tmin_c = -1e-3f;
    const float tmax_c = t_slack(best_t);
    const uint32_t w = q0.w;
    constexpr int kExpBias = RT_QEXP_MIN + 24; /* scales carry the 2^24 of the f16-subnormal planes */
    const float sx = __builtin_amdgcn_ldexpf(inv.x, (int)(w & 31u) + kExpBias);
    const float sy = __builtin_amdgcn_ldexpf(inv.y, (int)((w >> 5) & 31u) + kExpBias);
    const float sz = __builtin_amdgcn_ldexpf(inv.z, (int)((w >> 10) & 31u) + kExpBias);
    const float bx = __builtin_fmaf(__uint_as_float(q0.x), inv.x, -oi.x);
    const float by = __builtin_fmaf(__uint_as_float(q0.y), inv.y, -oi.y);
    const float bzo = __builtin_fmaf(__uint_as_float(q0.z), inv.z, -oi.z);
    const bool px = inv.x >= 0.0f, py = inv.y >= 0.0f, pz = inv.z >= 0.0f;
    const uint32_t nxw = px ? q1.x : q1.y, fxw = px ? q1.y : q1.x;
    const uint32_t nyw = py ? q1.z : q1.w, fyw = py ? q1.w : q1.z;
    const uint32_t nzw = pz ? q2.x : q2.y, fzw = pz ? q2.y : q2.x;
    int nhit = 0;
    /* the any-hit order's per-query terms (below): -1 selects the longest-segment key, and the
       penalty that sends boxes holding the ray origin last */
    const float lsel = longest ? -1.0f : 0.0f, pen = any_hit ? 1e4f : 0.0f;
    /* Plane bytes as f16 subnormals: v_perm_b32 spreads two bytes of a plane word into
       the low bytes of two 16-bit halves (0x00bb = b * 2^-24 as f16, exact), and
       v_fma_mix_f32 converts a half and does the FMA in one instruction, with the
       2^24 folded into the scale's exponent: (b * 2^-24) * (s * 2^24) + base is exactly
       fma(b, s, base) — the same bits as a byte convert + FMA, in 3/4 of the VALU. */
    const float sx24 = sx, sy24 = sy, sz24 = sz;
    const uint32_t nx01 = __builtin_amdgcn_perm(0u, nxw, 0x0c010c00u), nx23 = __builtin_amdgcn_perm(0u, nxw, 0x0c030c02u);
    const uint32_t ny01 = __builtin_amdgcn_perm(0u, nyw, 0x0c010c00u), ny23 = __builtin_amdgcn_perm(0u, nyw, 0x0c030c02u);
    const uint32_t nz01 = __builtin_amdgcn_perm(0u, nzw, 0x0c010c00u), nz23 = __builtin_amdgcn_perm(0u, nzw, 0x0c030c02u);
    const uint32_t fx01 = __builtin_amdgcn_perm(0u, fxw, 0x0c010c00u), fx23 = __builtin_amdgcn_perm(0u, fxw, 0x0c030c02u);
    const uint32_t fy01 = __builtin_amdgcn_perm(0u, fyw, 0x0c010c00u), fy23 = __builtin_amdgcn_perm(0u, fyw, 0x0c030c02u);
    const uint32_t fz01 = __builtin_amdgcn_perm(0u, fzw, 0x0c010c00u), fz23 = __builtin_amdgcn_perm(0u, fzw, 0x0c030c02u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float tn = __builtin_fmaxf(
            __builtin_fmaxf(__builtin_fmaf(half_of(i < 2 ? nx01 : nx23, i & 1), sx24, bx),
                            __builtin_fmaf(half_of(i < 2 ? ny01 : ny23, i & 1), sy24, by)),
            __builtin_fmaxf(__builtin_fmaf(half_of(i < 2 ? nz01 : nz23, i & 1), sz24, bzo), tmin_c));
        const float tf = __builtin_fminf(
            __builtin_fminf(__builtin_fmaf(half_of(i < 2 ? fx01 : fx23, i & 1), sx24, bx),
                            __builtin_fmaf(half_of(i < 2 ? fy01 : fy23, i & 1), sy24, by)),
            __builtin_fminf(__builtin_fmaf(half_of(i < 2 ? fz01 : fz23, i & 1), sz24, bzo), tmax_c));
        const bool h = tn <= tf; /* an unused slot's inverted box never passes */
        c[i] = (int)(i == 0 ? q3.x : i == 1 ? q3.y : i == 2 ? q3.z : q3.w);
        /* Any hit (the answer is order-free): children whose box holds the ray origin (the
           surface a shadow ray leaves, whose own triangles it cannot hit) are visited
           last, and a ray leaving the mesh (`longest`) takes the others by the length of
           its box segment, longest first — measured on the CPU model to find an occluder
           in the fewest steps; rays from the box walls keep nearest first. */
        const float key = __builtin_fmaf(lsel, tf, tn); /* tn - tf (longest) or tn, exactly */
        t[i] = h ? (tn <= 0.0f ? key + pen : key) : kInf;
        nhit += h ? 1 : 0;
    }
    /* Determinant cull (rt_quant.h): the node's normal box bounds d . N = det over its
       subtree; below 1e-4 (with the float error bound) no triangle can be accepted, so
       the subtree is skipped.  Culling only: the same results, fewer steps. */
    {
        /* v_perm_b32 picks, per axis, the hi byte (d >= 0) or the lo byte into `nb` (the box
           corner maximising d . N) and the other into `fb`; v_cvt_f32_ubyteN converts in
           place; the +128 byte bias folds into one per-ray term */
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
        /* bias rounding: |fl(128 sum d) - 128 sum d| <= 3u * 128 |d|_1, inside the margin */
        const float bound = __builtin_fmaf(__builtin_fmaxf(fhi, -flo) * nsc, 1.02f, 5e-7f * l1);
        if (bound < 1e-4f) nhit = 0;
    }
    if (nhit > 0) {
        cas(t[0], c[0], t[1], c[1]);
        cas(t[2], c[2], t[3], c[3]);
        cas(t[0], c[0], t[2], c[2]);
        cas(t[1], c[1], t[3], c[3]);
        cas(t[1], c[1], t[2], c[2]);
    }
    return nhit;
}

/* The shadow cache.  An any-hit answer is existential: an accepted triangle
   found in ANY subtree makes the ray occluded, whatever the full traversal would have met first,
   and `best` of such a query is only read as a flag.  So a lane keeps the node of one tree level
   (the cut: the nodes are numbered breadth-first, so a level is an index range [lo, lo + n))
   that its last occluded shadow query from a mesh hit entered last, and the pixel's next such
   query starts there instead of at the root (a try: `best` = RT_SC_TRYING until a hit); when that
   subtree holds no occluder the step that finds the stack empty restarts the query at the root,
   so an unoccluded answer always comes from the full traversal.
   The lane's word: 0 none, else the cut node's index in its level + 1 — 16 bits in LDS, written
   by the step under the lanes that enter the cut, so the stepping loop carries no register for
   it (k_tris clears it in the path advance, when such a query ends unoccluded).  Culling only:
   same frames, fewer steps.  n = 0: no cache. */
struct ShadowCut {
    uint32_t lo, n; /* the cut level's nodes (n <= 0xffff) */
    int root;       /* the shadow queries' root */
};
#define RT_SC_TRYING (-3) /* TravState::best of a try (any negative value: no hit yet) */
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) uint16_t lds_u16;
#else
typedef uint16_t lds_u16;
#endif

/* One step of the compressed 4-wide traversal (rt_quant.h).  Every lane fetches
   exactly one 64-B record per step — a node, or ONE triangle of its current leaf —
   with the same three dwordx4 loads, so a wave-step costs one memory round trip
   whatever mix of node and leaf lanes it holds (a leaf of k triangles takes k
   steps; the leaf cursor is the leaf code itself: first slot and remaining count).
   `sc` (k_tris): the lane's shadow-cache word, for its `longest` queries (any hit, from a mesh
   hit) — see ShadowCut. */
template <bool COUNT>
__device__ __forceinline__ bool trav_step_q(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                            TravState &s, Stack &stk, V3 o, V3 d, float tmin, bool any_hit,
                                            TravCounts &cnt, bool longest = false, lds_float *hn_out = nullptr,
                                            lds_u16 *sc = nullptr, ShadowCut cut = ShadowCut{0u, 0u, 0})
{
    const V3 inv = s.inv, oi = s.oi;
    const int node = s.node;
    const bool leaf = node < 0;
    /* wave-uniform: every lane's pushes and pops of this step stay in the LDS part
       of the stack (almost always), so they need no per-lane LDS/spill selection */
    const bool lds_only = !__any(stk.sp + 3 > RT_STACK_DEPTH);
    const uint32_t enc = (uint32_t)(~node);
    const uint4 *rec = leaf ? reinterpret_cast<const uint4 *>(tris) + 3 * (enc >> 3)
                            : reinterpret_cast<const uint4 *>(nodes) + 4 * node;
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u *vrec = reinterpret_cast<const v4u *>(rec);
    v4u w0 = vrec[0], w1 = vrec[1], w2 = vrec[2];
    /* the child links (d[12..15]) only for node lanes: the load runs under their exec mask,
       so leaf lanes add no addresses to it (-1 %) */
    v4u w3 = {0u, 0u, 0u, 0u};
    if (!leaf) w3 = vrec[3];
    /* Every lane's record arrives as whole dwordx4 loads issued together: without this
       the compiler narrows loads to the components each branch uses (x4 + x3 + x2 +
       dword) and sinks the child links below the box test, i.e. 5-6 vector-memory
       instructions per step instead of 4 (each costs the address path ~16 cycles per
       wave whatever its width) and a second dependent round trip for node lanes. */
    asm volatile("" : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3));
    const uint4 q0 = make_uint4(w0.x, w0.y, w0.z, w0.w), q1 = make_uint4(w1.x, w1.y, w1.z, w1.w);
    const uint4 q2 = make_uint4(w2.x, w2.y, w2.z, w2.w);
    const uint4 q3 = make_uint4(w3.x, w3.y, w3.z, w3.w);
    if (leaf) {
        if (COUNT) {
            cnt.tests++;
            cnt.leaves++;
        }
        const float4 a = make_float4(__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z),
                                     __uint_as_float(q0.w));
        const float4 b = make_float4(__uint_as_float(q1.x), __uint_as_float(q1.y), __uint_as_float(q1.z), 0.0f);
        const float4 c = make_float4(__uint_as_float(q2.x), __uint_as_float(q2.y), __uint_as_float(q2.z), 0.0f);
        float t = 0.0f;
        const bool h = mt_test(o, d, a, b, c, t);
        const int slot = (int)(enc >> 3);
        if (h) {
            if (any_hit) {
                if (t < s.best_t && t > tmin) {
                    s.best = slot;
                    return true;
                }
            } else if (!(t < tmin)) {
                /* the accept rule t < best_t || (t == best_t && orig > best_orig): the best hit's
                   original index is read back from its record on the rare exact tie instead of
                   being carried in a register (which the compiler spilled on every step) */
                bool acc = t < s.best_t;
                if (!acc && t == s.best_t)
                    acc = s.best < 0 || __float_as_int(a.w) > __float_as_int(tris[3 * s.best].w);
                if (acc) {
                    s.best = slot;
                    s.best_t = t;
                    if (hn_out) { /* the hit's unnormalised normal for the shading (rtcommon.h:389) */
                        const V3 n = cross3(v3(c.x, c.y, c.z), v3(b.x, b.y, b.z));
                        hn_out[0] = n.x;
                        hn_out[RT_BLOCK] = n.y;
                        hn_out[2 * RT_BLOCK] = n.z;
                    }
                }
            }
        }
        /* a camera candidate list (k_pixel_lists) is sorted, r1.w = the next candidate's
           earliest accept t: past the best hit, nothing later can be accepted (tree leaves: 0) */
        if (!any_hit && s.best_t < __uint_as_float(q1.w)) return true;
        if (enc & 7u) { /* next triangle of this leaf */
            s.node = ~(int)((((enc >> 3) + 1u) << 3) | ((enc & 7u) - 1u));
            return false;
        }
    } else {
        if (COUNT) cnt.nodes++;
        if (sc && longest) { /* the cut node this descent is under */
            const uint32_t r = (uint32_t)node - cut.lo;
            if (r < cut.n) *sc = (uint16_t)(r + 1u);
        }
        float t[4];
        int c[4];
        const int nhit = node_children(q0, q1, q2, q3, inv, oi, d, s.best_t, any_hit, longest, t, c);
        if (nhit > 0) {
            if (lds_only) {
                /* the nhit - 1 farther hits, farthest first, written unconditionally at
                   sp, sp+1, sp+2 (slots above the new top hold junk) */
                const int v0 = nhit >= 4 ? c[3] : (nhit == 3 ? c[2] : c[1]);
                const int v1 = nhit >= 4 ? c[2] : c[1];
                lds_int *top = stk.lds + stk.sp * RT_BLOCK;
                top[0] = v0;
                top[RT_BLOCK] = v1;
                top[2 * RT_BLOCK] = c[1];
                stk.sp += nhit - 1;
            } else {
                if (nhit >= 4) stk.push(c[3]);
                if (nhit >= 3) stk.push(c[2]);
                if (nhit >= 2) stk.push(c[1]);
            }
            s.node = c[0];
            return false;
        }
    }
    if (stk.sp == 0) {
        if (sc && s.best == RT_SC_TRYING) { /* no occluder under the cached node: the full traversal, from
                                               the next step on (tmax unchanged) */
            s.best = -1;
            s.node = cut.root;
            return false;
        }
        return true;
    }
    if (lds_only) s.node = stk.lds[--stk.sp * RT_BLOCK];
    else s.node = stk.pop();
    return false;
}


/* One traversal step; returns true when the query is complete.  Closest hit:
   the result equals the reference's linear loop (minimum t, ties to the highest
   original index — rtcommon.h:39-52 with intersects_triangle's `t > tmax`
   rejection).  Any hit: best >= 0 iff some triangle has tmin < t < tmax
   (rtcommon.h:59-68). */
template <int TRAV, bool COUNT>
__device__ __forceinline__ bool trav_step(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                          TravState &s, Stack &stk, V3 o, V3 d, float tmin, bool any_hit,
                                          TravCounts &cnt, bool longest = false, lds_float *hn_out = nullptr,
                                          lds_u16 *sc = nullptr, ShadowCut cut = ShadowCut{0u, 0u, 0})
{
    if (TRAV == RT_TRAV_BVH4Q)
        return trav_step_q<COUNT>(nodes, tris, s, stk, o, d, tmin, any_hit, cnt, longest, hn_out, sc, cut);
    const float tmin_c = -1e-3f;
    const V3 inv = s.inv, oi = s.oi;
    int node = s.node;
    if (node >= 0) {
        if (COUNT) cnt.nodes++;
        const float tmax_c = t_slack(s.best_t);
        {
            /* 4-wide: near/far slab planes picked by the direction signs, so each
               child costs 6 FMAs + max3/min3 and no min/max pairs. */
            const int nxo = inv.x >= 0.0f ? 0 : 1, nyo = inv.y >= 0.0f ? 2 : 3, nzo = inv.z >= 0.0f ? 4 : 5;
            const int fxo = 1 - nxo, fyo = 5 - nyo, fzo = 9 - nzo;
            const float4 *nd = nodes + 8 * node;
            const float4 nx = nd[nxo], fx = nd[fxo], ny = nd[nyo], fy = nd[fyo], nz = nd[nzo], fz = nd[fzo];
            const float4 cc = nd[6];
            float t[4];
            int c[4];
            const float nxs[4] = {nx.x, nx.y, nx.z, nx.w}, fxs[4] = {fx.x, fx.y, fx.z, fx.w};
            const float nys[4] = {ny.x, ny.y, ny.z, ny.w}, fys[4] = {fy.x, fy.y, fy.z, fy.w};
            const float nzs[4] = {nz.x, nz.y, nz.z, nz.w}, fzs[4] = {fz.x, fz.y, fz.z, fz.w};
            const int cs[4] = {__float_as_int(cc.x), __float_as_int(cc.y), __float_as_int(cc.z),
                               __float_as_int(cc.w)};
            int nhit = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float tn = __builtin_fmaxf(
                    __builtin_fmaxf(__builtin_fmaf(nxs[i], inv.x, -oi.x), __builtin_fmaf(nys[i], inv.y, -oi.y)),
                    __builtin_fmaxf(__builtin_fmaf(nzs[i], inv.z, -oi.z), tmin_c));
                const float tf = __builtin_fminf(
                    __builtin_fminf(__builtin_fmaf(fxs[i], inv.x, -oi.x), __builtin_fmaf(fys[i], inv.y, -oi.y)),
                    __builtin_fminf(__builtin_fmaf(fzs[i], inv.z, -oi.z), tmax_c));
                const bool h = (tn <= tf) && (cs[i] != RT_EMPTY_CHILD);
                t[i] = h ? tn : kInf;
                c[i] = cs[i];
                nhit += h ? 1 : 0;
            }
            if (nhit > 0) {
                /* sort the (entry distance, child) pairs: misses (inf) sink to the end */
                cas(t[0], c[0], t[1], c[1]);
                cas(t[2], c[2], t[3], c[3]);
                cas(t[0], c[0], t[2], c[2]);
                cas(t[1], c[1], t[3], c[3]);
                cas(t[1], c[1], t[2], c[2]);
                if (nhit >= 4) stk.push(c[3]);
                if (nhit >= 3) stk.push(c[2]);
                if (nhit >= 2) stk.push(c[1]);
                s.node = c[0];
                return false;
            }
        }
    } else {
        const int enc = ~node;
        if (COUNT) cnt.leaves++;
        if (leaf_tests<COUNT>(tris, enc >> 3, (enc & 7) + 1, o, d, tmin, s.best_t, any_hit, s.best, s.best_orig,
                              s.best_t, cnt))
            return true;
    }
    if (stk.sp == 0) return true;
    s.node = stk.pop();
    return false;
}

/* One ray query.  Closest hit (any_hit = false): returns the leaf-order slot of
   the hit (or -1) with t in tmax; the result equals the reference's linear
   loop: minimum t, ties to the highest original index (rtcommon.h:39-52 with
   intersects_triangle's `t > tmax` rejection).  Any hit: returns >= 0 iff some
   triangle has tmin < t < tmax (rtcommon.h:59-68). */
template <int TRAV, bool COUNT>
__device__ __forceinline__ int traverse(const float4 *__restrict__ nodes, const float4 *__restrict__ tris,
                                        uint32_t n_tris, V3 o, V3 d, float tmin, float &tmax, bool any_hit,
                                        Stack &stk, TravCounts &cnt)
{
    int best = -1;
    int best_orig = -1;
    float best_t = tmax;
    if (TRAV == RT_TRAV_LINEAR) {
        /* The reference algorithm: every triangle, in a wave-uniform loop (the
           slot index is uniform, so the records come in through scalar loads). */
        bool live = true;
        for (uint32_t s = 0; s < n_tris; ++s) {
            if (live) {
                const float4 a = tris[3 * s], b = tris[3 * s + 1], c = tris[3 * s + 2];
                float t;
                if (COUNT) cnt.tests++;
                if (mt_test(o, d, a, b, c, t)) {
                    if (any_hit) {
                        if (t < tmax && t > tmin) {
                            best = (int)s;
                            live = false;
                        }
                    } else {
                        const int orig = __float_as_int(a.w);
                        if (!(t < tmin) && (t < best_t || (t == best_t && orig > best_orig))) {
                            best = (int)s;
                            best_orig = orig;
                            best_t = t;
                        }
                    }
                }
            }
            if (!__any(live)) break;
        }
        if (!any_hit) tmax = best_t;
        return best;
    }

    TravState st;
    trav_begin(st, stk, o, d, tmax);
    while (!trav_step<TRAV, COUNT>(nodes, tris, st, stk, o, d, tmin, any_hit, cnt)) {
    }
    if (!any_hit) tmax = st.best_t;
    return st.best;
}

} // namespace

#endif /* RT_TRAVERSE_H */
