/*
 * rt_build_gpu.hip — BVH build on the GPU ("the step before the
 * path").  Produces the same 4-wide layouts the traversal reads (rt_internal.h: 128-B
 * float nodes (the full-precision traversal), 64-B compressed nodes for the
 * default traversal) and the leaf-ordered triangle records, from the mesh arrays of
 * raytrace_tris (tri_verts / tri_vert_idx, raytracer.cl:184-188).
 *
 *   0. (RT_BUILD_OPT_LIGHTS) one class per triangle by the rules of
 *      rt_tri_rules.h — left out, parked, possible occluder — and the triangle list in class
 *      order by one prefix sum; steps 1-5 then run over a list: once over the kept triangles
 *      (the closest-hit tree), and once each over the occluders (A) and the parked (B) for the
 *      shadow tree, whose root has exactly these two children;
 *   1. per triangle: padded box (the host builder's pad: ext/512 + 1e-6(1+|coord|)) and
 *      centroid; centroid bounds by ordered-integer atomics;
 *   2. 63-bit Morton codes (21 bits per axis) of the centroids, radix-sorted (hipCUB)
 *      with the triangle index as payload;
 *   3. binary radix tree over the sorted codes (Karras 2012; equal codes broken by the
 *      slot index), one thread per inner node; every node covers a contiguous slot range;
 *   4. boxes bottom-up: one thread per leaf climbs, the second arrival at a node merges;
 *   3'-4'. (RT_BUILD_GPU_PLOC, instead of 3-4) PLOC: the sorted triangles are clusters; per
 *      round every cluster finds the neighbour within 16 positions whose union with it has
 *      the smallest area, pairs that chose each other merge into a node, a prefix sum
 *      numbers the nodes and compacts the array; flat launches, the count read back once
 *      per round, halving rounds past a cap;
 *   5. collapse to the 4-wide tree top-down, one launch per level (largest-area child
 *      expanded first, as the host collapse; a subtree of <= kLeafMax triangles becomes a
 *      leaf over its slot range, or over its gathered slots under PLOC), nodes numbered
 *      breadth-first (root 0);
 *   5a-5b. (RT_COLLAPSE_SAH, instead of 5's rule) the host collapse's dynamic
 *      programming: bottom-up per binary node the cost of standing for 1..4 children of a wide
 *      node, as a leaf, a node of its own or dissolved into its parent's; top-down the same
 *      launches per level with the children the costs chose;
 *   6. quantisation of every node (same rounding rule as rt_bvh.cpp) and the triangle
 *      records in slot order, e1/e2 formed by the reference's get_triangle subtraction.
 *
 * The traversal contract is unchanged (conservative boxes, the accept rule in the leaf
 * test), so results equal the linear loop exactly; only the tree shape — and therefore
 * speed — differs from the host SAH build.
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "rt_internal.h"
#include "rt_quant.h"
#include "rt_tri_rules.h"

#pragma clang fp contract(off)

namespace {

constexpr int kB = 256;
constexpr uint32_t kLeafMax = 4; /* largest slot range emitted as one leaf */

__device__ __forceinline__ uint32_t f2key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

/* 1. padded triangle boxes + centroids (by triangle index); bounds[0..2] = min key, [3..5] = max key */
__global__ void k_prep(const float *__restrict__ verts, const int32_t *__restrict__ idx,
                       const uint32_t *__restrict__ sub, uint32_t n, float *__restrict__ tbox,
                       float *__restrict__ cent, uint32_t *__restrict__ bounds)
{
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    float c[3] = {0, 0, 0};
    bool ok = i < n;
    if (ok) {
        const uint32_t t = sub ? sub[i] : i; /* a part of the mesh: the triangles its list names */
        float lo[3], hi[3], maxabs = 0.0f;
        for (int a = 0; a < 3; ++a) {
            lo[a] = INFINITY;
            hi[a] = -INFINITY;
        }
        for (int k = 0; k < 3; ++k) {
            const float *p = verts + 3ull * (uint32_t)idx[3ull * t + k];
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(lo[a], p[a]);
                hi[a] = fmaxf(hi[a], p[a]);
                maxabs = fmaxf(maxabs, fabsf(p[a]));
            }
        }
        float ext = 0.0f;
        for (int a = 0; a < 3; ++a) ext = fmaxf(ext, hi[a] - lo[a]);
        const float pad = ext * (1.0f / 512.0f) + 1e-6f * (1.0f + maxabs);
        for (int a = 0; a < 3; ++a) {
            c[a] = 0.5f * (lo[a] + hi[a]);
            cent[3ull * t + a] = c[a];
            tbox[6ull * t + a] = lo[a] - pad;
            tbox[6ull * t + 3 + a] = hi[a] + pad;
        }
    }
    /* block reduction of the centroid bounds, one atomic per block and bound */
    __shared__ uint32_t s_lo[3], s_hi[3];
    if (threadIdx.x < 3) {
        s_lo[threadIdx.x] = 0xFFFFFFFFu;
        s_hi[threadIdx.x] = 0u;
    }
    __syncthreads();
    if (ok)
        for (int a = 0; a < 3; ++a) {
            atomicMin(&s_lo[a], f2key(c[a]));
            atomicMax(&s_hi[a], f2key(c[a]));
        }
    __syncthreads();
    if (threadIdx.x < 3) {
        atomicMin(&bounds[threadIdx.x], s_lo[threadIdx.x]);
        atomicMax(&bounds[3 + threadIdx.x], s_hi[threadIdx.x]);
    }
}

__device__ __forceinline__ uint64_t spread21(uint64_t v)
{
    v &= 0x1FFFFFull;
    v = (v | (v << 32)) & 0x1F00000000FFFFull;
    v = (v | (v << 16)) & 0x1F0000FF0000FFull;
    v = (v | (v << 8)) & 0x100F00F00F00F00Full;
    v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

/* 2. Morton codes + identity payload */
__global__ void k_morton(const float *__restrict__ cent, const uint32_t *__restrict__ sub, uint32_t n,
                         const uint32_t *__restrict__ bounds, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = sub ? sub[i] : i;
    uint64_t code = 0;
    for (int a = 0; a < 3; ++a) {
        const float lo = key2f(bounds[a]), hi = key2f(bounds[3 + a]);
        const float ext = hi - lo;
        float u = ext > 0.0f ? (cent[3ull * t + a] - lo) / ext : 0.0f;
        u = fminf(fmaxf(u, 0.0f), 1.0f);
        const uint64_t q = (uint64_t)fminf(u * 2097152.0f, 2097151.0f);
        code |= spread21(q) << (2 - a);
    }
    keys[i] = code;
    vals[i] = t;
}

/* 3. radix tree.  Inner node i in [0, n-2]; child c >= 0 inner, c < 0 leaf ~slot. */
__device__ __forceinline__ int delta(const uint64_t *__restrict__ k, int n, int i, int j)
{
    if (j < 0 || j >= n) return -1;
    const uint64_t a = k[i], b = k[j];
    if (a == b) return 64 + __clz((uint32_t)i ^ (uint32_t)j);
    return __clzll((long long)(a ^ b));
}

__global__ void k_radix_tree(const uint64_t *__restrict__ k, int n, int2 *__restrict__ child,
                             int2 *__restrict__ range, int *__restrict__ parent_inner, int *__restrict__ parent_leaf)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n - 1) return;
    const int d = (delta(k, n, i, i + 1) - delta(k, n, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = delta(k, n, i, i - d);
    int lmax = 2;
    while (delta(k, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(k, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta(k, n, i, j);
    int s = 0;
    int t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(k, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int g = i + s * d + (d < 0 ? -1 : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int left = (lo == g) ? ~g : g;
    const int right = (hi == g + 1) ? ~(g + 1) : g + 1;
    child[i] = make_int2(left, right);
    range[i] = make_int2(lo, hi);
    if (left >= 0) parent_inner[left] = i;
    else parent_leaf[~left] = i;
    if (right >= 0) parent_inner[right] = i;
    else parent_leaf[~right] = i;
}

/* 4. bottom-up boxes */
__global__ void k_boxes(const float *__restrict__ tbox, const uint32_t *__restrict__ perm, int n,
                        const int2 *__restrict__ child, const int *__restrict__ parent_inner,
                        const int *__restrict__ parent_leaf, float *__restrict__ nbox, int *__restrict__ flags)
{
    const int s = blockIdx.x * kB + threadIdx.x;
    if (s >= n || n < 2) return;
    int node = parent_leaf[s];
    while (node >= 0) {
        __threadfence();
        if (atomicAdd(&flags[node], 1) == 0) return; /* the sibling finishes this node */
        __threadfence();
        const int2 c = child[node];
        float b[6];
        for (int q = 0; q < 2; ++q) {
            const int ci = q ? c.y : c.x;
            const float *src = ci >= 0 ? nbox + 6ull * ci : tbox + 6ull * perm[~ci];
            /* the sibling's box was written by another workgroup: L1-bypassing loads */
            float v[6];
            for (int a = 0; a < 6; ++a)
                v[a] = __uint_as_float(__hip_atomic_load(reinterpret_cast<const uint32_t *>(src + a),
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (q == 0)
                for (int a = 0; a < 6; ++a) b[a] = v[a];
            else
                for (int a = 0; a < 3; ++a) {
                    b[a] = fminf(b[a], v[a]);
                    b[3 + a] = fmaxf(b[3 + a], v[3 + a]);
                }
        }
        for (int a = 0; a < 6; ++a) nbox[6ull * node + a] = b[a];
        node = node == 0 ? -1 : parent_inner[node];
    }
}

__device__ __forceinline__ float box_area(const float *b)
{
    const float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
    if (!(dx >= 0.0f) || !(dy >= 0.0f) || !(dz >= 0.0f)) return 0.0f;
    return 2.0f * (dx * dy + dy * dz + dz * dx);
}

/* 3'-4'. PLOC (Meister & Bittner 2018): the binary tree by rounds of merges of mutual nearest
   neighbours in the sorted order, instead of 3-4.  A cluster is (id, box): id >= 0 a binary
   node, id < 0 the leaf ~slot.  DESIGN.md §4.6a has the rule. */
constexpr int kPlocR = 16; /* search radius, in positions of the cluster array */

__global__ void k_ploc_init(const float *__restrict__ tbox, const uint32_t *__restrict__ perm, int n,
                            int *__restrict__ cid, float *__restrict__ cbox)
{
    const int s = blockIdx.x * kB + threadIdx.x;
    if (s >= n) return;
    cid[s] = ~s;
    const float *src = tbox + 6ull * perm[s];
    for (int a = 0; a < 6; ++a) cbox[6ull * s + a] = src[a];
}

/* nn[i]: among the positions j != i within kPlocR of i, the one with the smallest
   (area of the union, j == i ^ 1 ? 0 : 1, j).  A block stages its positions' boxes and a halo
   of kPlocR on each side in LDS, one array per plane so that a wave's reads are consecutive.
   halving: nn[i] = i ^ 1 (or none, -1, for the last of an odd count). */
__global__ __launch_bounds__(kB) void k_ploc_nn(const float *__restrict__ cbox, int C, int halving,
                                                 int *__restrict__ nn)
{
    constexpr int kW = kB + 2 * kPlocR;
    __shared__ float s_box[6][kW];
    const int i = blockIdx.x * kB + threadIdx.x;
    if (halving) { /* the same in every thread of the launch */
        if (i < C) nn[i] = (i ^ 1) < C ? (i ^ 1) : -1;
        return;
    }
    const int base = blockIdx.x * kB - kPlocR; /* position of s_box[.][0] */
    const int first = base < 0 ? 0 : base;
    const int last = base + kW < C ? base + kW : C; /* staged positions: [first, last) */
    const float *src = cbox + 6ull * (uint32_t)first;
    for (int f = threadIdx.x; f < 6 * (last - first); f += kB) s_box[f % 6][first - base + f / 6] = src[f];
    __syncthreads();
    if (i >= C) return;
    const int e0 = threadIdx.x + kPlocR;
    float b[6];
    for (int a = 0; a < 6; ++a) b[a] = s_box[a][e0];
    int best_j = -1;
    float best_d = 0.0f;
    for (int k = -kPlocR; k <= kPlocR; ++k) {
        const int j = i + k;
        if (k == 0 || j < 0 || j >= C) continue;
        float u[6];
        for (int a = 0; a < 3; ++a) {
            u[a] = fminf(b[a], s_box[a][e0 + k]);
            u[3 + a] = fmaxf(b[3 + a], s_box[3 + a][e0 + k]);
        }
        const float d = box_area(u);
        if (best_j < 0 || d < best_d || (d == best_d && j == (i ^ 1))) {
            best_d = d;
            best_j = j;
        }
    }
    nn[i] = best_j;
}

/* A pair is merged when each is the other's choice; its lower position (the leader) keeps
   the place.  flags[i] = leader << 32 | kept: one exclusive sum numbers the new nodes and
   the surviving positions. */
__global__ void k_ploc_flags(const int *__restrict__ nn, int C, uint64_t *__restrict__ flags)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= C) return;
    const int j = nn[i];
    const bool mutual = j >= 0 && j < C && nn[j] == i;
    flags[i] = ((uint64_t)(mutual && i < j) << 32) | (uint64_t)!(mutual && i > j);
}

/* The round's merges and the compaction: a leader at position i makes node K + (leaders before
   i) with the children (cid[i], cid[nn[i]]); every kept cluster moves to (kept before it). */
__global__ void k_ploc_merge(const int *__restrict__ cid, const float *__restrict__ cbox,
                             const int *__restrict__ nn, const uint64_t *__restrict__ flags,
                             const uint64_t *__restrict__ scan, int C, int K, int n_inner, int *__restrict__ cid_out,
                             float *__restrict__ cbox_out, int2 *__restrict__ child, float *__restrict__ nbox,
                             uint32_t *__restrict__ nsize, uint32_t *__restrict__ c_out)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= C) return;
    const uint64_t fl = flags[i], sc = scan[i];
    const uint32_t pos = (uint32_t)sc;
    if (i == C - 1) *c_out = pos + (uint32_t)(fl & 1u);
    if (!(fl & 1u)) return;
    float b[6];
    for (int a = 0; a < 6; ++a) b[a] = cbox[6ull * i + a];
    int id = cid[i];
    if (fl >> 32) {
        const int j = nn[i];
        const int node = K + (int)(sc >> 32);
        if (node >= n_inner) return; /* cannot happen: n - 1 merges in all (the host checks the count) */
        const int idj = cid[j];
        for (int a = 0; a < 3; ++a) {
            b[a] = fminf(b[a], cbox[6ull * j + a]);
            b[3 + a] = fmaxf(b[3 + a], cbox[6ull * j + 3 + a]);
        }
        child[node] = make_int2(id, idj);
        for (int a = 0; a < 6; ++a) nbox[6ull * node + a] = b[a];
        nsize[node] = (id >= 0 ? nsize[id] : 1u) + (idj >= 0 ? nsize[idj] : 1u);
        id = node;
    }
    cid_out[pos] = id;
    for (int a = 0; a < 6; ++a) cbox_out[6ull * pos + a] = b[a];
}

struct Frontier {
    int bin;   /* binary inner node (or ~slot for a single-triangle mesh) */
    int out;   /* 4-wide node index */
    int stack; /* traversal stack entries live on entry */
};

/* 5. one level of the top-down collapse.  kPloc = false: the radix tree, whose nodes cover
   contiguous slot ranges (`range`).  kPloc = true: the PLOC tree, whose nodes cover any set of
   slots: a subtree's triangle count is read from `nsize`, and a leaf's slots are gathered by a
   walk of its (at most 2 kLeafMax - 1) nodes, left child first. */
template <bool kPloc>
__global__ void k_collapse(const Frontier *__restrict__ cur, const uint32_t *__restrict__ n_cur,
                           Frontier *__restrict__ next, uint32_t *__restrict__ n_next, uint32_t *__restrict__ n_nodes,
                           uint32_t *__restrict__ max_stack, const int2 *__restrict__ child,
                           const int2 *__restrict__ range, const uint32_t *__restrict__ nsize,
                           const float *__restrict__ nbox, const float *__restrict__ tbox,
                           const uint32_t *__restrict__ perm, int n, float *__restrict__ nodes4,
                           uint32_t *__restrict__ n_tris_out, uint32_t *__restrict__ perm2)
{
    const uint32_t e = blockIdx.x * kB + threadIdx.x;
    if (e >= *n_cur) return;
    const Frontier f = cur[e];
    int kids[4] = {0, 0, 0, 0};
    int nk = 0;
    auto size_of = [&](int c) -> int {
        if (c < 0) return 1;
        if constexpr (kPloc) return (int)nsize[c];
        else return range[c].y - range[c].x + 1;
    };
    auto expandable = [&](int c) -> bool { return c >= 0 && size_of(c) > (int)kLeafMax; };
    if (f.bin < 0 || n < 2 || size_of(f.bin) <= (int)kLeafMax) {
        kids[nk++] = f.bin; /* the whole (small) mesh as one leaf */
    } else {
        kids[nk++] = child[f.bin].x;
        kids[nk++] = child[f.bin].y;
        while (nk < 4) {
            int best = -1;
            float best_a = -1.0f;
            for (int i = 0; i < nk; ++i)
                if (expandable(kids[i])) {
                    const float a = box_area(nbox + 6ull * kids[i]);
                    if (a > best_a) {
                        best_a = a;
                        best = i;
                    }
                }
            if (best < 0) break;
            const int c = kids[best];
            kids[best] = child[c].x;
            kids[nk++] = child[c].y;
        }
    }
    const int stk = f.stack + (nk > 0 ? nk - 1 : 0);
    atomicMax(max_stack, (uint32_t)stk);
    /* inner children get consecutive node indices, leaf children consecutive
       triangle slots (rt_quant.h), allocated as one block each */
    int n_in = 0;
    uint32_t n_leaf_tris = 0;
    for (int k = 0; k < nk; ++k) {
        const int c = kids[k];
        if (c >= 0 && n >= 2 && expandable(c)) ++n_in;
        else n_leaf_tris += (c < 0 && n >= 2) ? 1u : (n >= 2 && c >= 0 ? (uint32_t)size_of(c) : (uint32_t)n);
    }
    const uint32_t node_base = n_in ? atomicAdd(n_nodes, (uint32_t)n_in) : 0u;
    const uint32_t tri_base = n_leaf_tris ? atomicAdd(n_tris_out, n_leaf_tris) : 0u;
    uint32_t next_node = node_base, next_tri = tri_base;
    float *nd = nodes4 + 32ull * f.out;
    for (int k = 0; k < 4; ++k) {
        int32_t code = RT_EMPTY_CHILD;
        float b[6] = {0, 0, 0, 0, 0, 0};
        if (k < nk) {
            const int c = kids[k];
            if (c >= 0 && n >= 2 && expandable(c)) {
                for (int a = 0; a < 6; ++a) b[a] = nbox[6ull * c + a];
                const uint32_t id = next_node++;
                code = (int32_t)id;
                const uint32_t q = atomicAdd(n_next, 1u);
                next[q] = Frontier{c, (int)id, stk};
            } else {
                /* a leaf: one triangle (binary leaf), a small subtree's slot range, or
                   the whole mesh of <= kLeafMax triangles */
                uint32_t first_old = 0, count = (uint32_t)n;
                if (c < 0 && n >= 2) {
                    first_old = (uint32_t)(~c);
                    count = 1;
                    for (int a = 0; a < 6; ++a) b[a] = tbox[6ull * perm[first_old] + a];
                } else if (n >= 2) {
                    if constexpr (!kPloc) first_old = (uint32_t)range[c].x;
                    count = (uint32_t)size_of(c);
                    for (int a = 0; a < 6; ++a) b[a] = nbox[6ull * c + a];
                } else {
                    for (int a = 0; a < 6; ++a) b[a] = tbox[6ull * perm[0] + a];
                }
                const uint32_t first = next_tri;
                next_tri += count;
                if (kPloc && c >= 0 && n >= 2) {
                    /* count <= kLeafMax: at most 2 kLeafMax - 1 nodes, the stack never holds
                       more than kLeafMax of them */
                    int stack[kLeafMax + 1], sp = 0;
                    uint32_t q = 0;
                    stack[sp++] = c;
                    for (uint32_t it = 0; it < 2 * kLeafMax - 1 && sp > 0; ++it) {
                        const int x = stack[--sp];
                        if (x < 0) {
                            if (q < count) perm2[first + q++] = (uint32_t)(~x);
                        } else if (sp + 2 <= (int)kLeafMax + 1) {
                            stack[sp++] = child[x].y;
                            stack[sp++] = child[x].x;
                        }
                    }
                } else {
                    for (uint32_t q = 0; q < count; ++q) perm2[first + q] = first_old + q;
                }
                code = ~(int32_t)((first << 3) | (count - 1));
            }
        }
        nd[0 + k] = b[0];
        nd[4 + k] = b[3];
        nd[8 + k] = b[1];
        nd[12 + k] = b[4];
        nd[16 + k] = b[2];
        nd[20 + k] = b[5];
        nd[24 + k] = __int_as_float(code);
        nd[28 + k] = 0.0f;
    }
}

/* ---- RT_COLLAPSE_SAH: the collapse by dynamic programming, as the host's ----
   Per binary node c, D[c][j] (j = 1..4) is the cost of presenting c's triangles as at most j
   children of a wide node, a step being one wide-node visit or one triangle of a visited leaf,
   weighted by the box's area.  The word beside it: bits 0-5 split[2..4] (2 bits each: how many of
   the j children the left child takes, 0: c stays whole), bit 6 as_leaf, bits 8-9 a* (the left
   child's share when c itself is the wide node), bits 12-14 min(size, 7). */
constexpr uint32_t kWordLeaf = 1u << 6;

__device__ __forceinline__ float ld_agent(const float *p)
{
    return __uint_as_float(__hip_atomic_load(reinterpret_cast<const uint32_t *>(p), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_agent(float *p, float v)
{
    __hip_atomic_store(reinterpret_cast<uint32_t *>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* the parent links of the PLOC tree (the radix tree's come from k_radix_tree); the root keeps -1 */
__global__ void k_parents(const int2 *__restrict__ child, int n_inner, int *__restrict__ parent_inner,
                          int *__restrict__ parent_leaf)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n_inner) return;
    const int2 c = child[i];
    if (c.x >= 0) parent_inner[c.x] = i;
    else parent_leaf[~c.x] = i;
    if (c.y >= 0) parent_inner[c.y] = i;
    else parent_leaf[~c.y] = i;
}

/* 5a. the bottom-up pass, by k_boxes' climb: one thread per leaf slot, the second arrival at a
   node computes it from its finished children.  No thread waits.  A node's values depend on its
   children's alone, so they are a function of the input.  range (radix tree) or nsize (PLOC)
   gives a node's triangle count. */
__global__ void k_collapse_cost(const float *__restrict__ tbox, const uint32_t *__restrict__ perm, int n,
                                const int2 *__restrict__ child, const int2 *__restrict__ range,
                                const uint32_t *__restrict__ nsize, const int *__restrict__ parent_inner,
                                const int *__restrict__ parent_leaf, const float *__restrict__ nbox,
                                int *__restrict__ flags, float *__restrict__ D, uint32_t *__restrict__ word)
{
    const int s = blockIdx.x * kB + threadIdx.x;
    if (s >= n || n < 2) return;
    int node = parent_leaf[s];
    while (node >= 0 && node < n - 1) {
        __threadfence();
        if (atomicAdd(&flags[node], 1) == 0) return; /* the sibling finishes this node */
        __threadfence();
        const int2 c = child[node];
        float dl[4], dr[4];
        for (int q = 0; q < 2; ++q) {
            const int ci = q ? c.y : c.x;
            float *d = q ? dr : dl;
            if (ci >= 0) { /* another workgroup may have written them: L1-bypassing loads */
                for (int a = 0; a < 4; ++a) d[a] = ld_agent(D + 4ull * ci + a);
            } else {
                const float ar = box_area(tbox + 6ull * perm[~ci]);
                for (int a = 0; a < 4; ++a) d[a] = ar;
            }
        }
        const uint32_t size = nsize ? nsize[node] : (uint32_t)(range[node].y - range[node].x + 1);
        const float area = box_area(nbox + 6ull * node);
        const bool small = size <= kLeafMax;
        const float leaf_c = small ? area * (float)size : INFINITY;
        float best_int = dl[0] + dr[2];
        uint32_t a_star = 1;
        for (int a = 2; a <= 3; ++a) {
            const float v = dl[a - 1] + dr[3 - a];
            if (v < best_int) {
                best_int = v;
                a_star = (uint32_t)a;
            }
        }
        const float inner_c = area + best_int;
        const bool as_leaf = small && leaf_c <= inner_c;
        float d[4];
        d[0] = as_leaf ? leaf_c : inner_c;
        uint32_t w = (as_leaf ? kWordLeaf : 0u) | (a_star << 8) | ((size < 7u ? size : 7u) << 12);
        for (int j = 2; j <= 4; ++j) {
            float best = d[0];
            uint32_t sp = 0;
            for (int a = 1; a < j; ++a) {
                const float v = dl[a - 1] + dr[j - a - 1];
                if (v < best) {
                    best = v;
                    sp = (uint32_t)a;
                }
            }
            d[j - 1] = best;
            w |= sp << (2 * (j - 2));
        }
        for (int a = 0; a < 4; ++a) st_agent(D + 4ull * node + a, d[a]);
        word[node] = w;
        node = parent_inner[node];
    }
}

/* 5b. one level of the top-down pass, the shape of k_collapse: the wide node over binary node b
   has the children expand(left, a*) ++ expand(right, 4 - a*), where expand(c, j) is [c] when
   split[c][j] is 0 (or c is a binary leaf) and expand(left, s) ++ expand(right, j - s) otherwise.
   A child is an inner child exactly when it is a binary inner node that is not as_leaf; any other
   is a leaf of its <= kLeafMax slots, gathered left child first. */
__global__ void k_collapse_sah(const Frontier *__restrict__ cur, const uint32_t *__restrict__ n_cur,
                               Frontier *__restrict__ next, uint32_t *__restrict__ n_next, uint32_t *__restrict__ n_nodes,
                               uint32_t *__restrict__ max_stack, const int2 *__restrict__ child,
                               const uint32_t *__restrict__ word, const float *__restrict__ nbox,
                               const float *__restrict__ tbox, const uint32_t *__restrict__ perm, int n,
                               float *__restrict__ nodes4, uint32_t *__restrict__ n_tris_out, uint32_t *__restrict__ perm2)
{
    const uint32_t e = blockIdx.x * kB + threadIdx.x;
    if (e >= *n_cur) return;
    const Frontier f = cur[e];
    int kids[4] = {0, 0, 0, 0};
    int nk = 0;
    if (f.bin < 0 || n < 2) {
        kids[nk++] = f.bin; /* the single triangle */
    } else {
        /* the sum of the shares on the stack and the children made is 4, every share >= 1: at
           most 4 entries, at most 6 nodes popped */
        int sc[4], sj[4], sp = 0;
        const int2 ch = child[f.bin];
        int a = (int)((word[f.bin] >> 8) & 3u);
        a = a < 1 ? 1 : a;
        sc[sp] = ch.y, sj[sp++] = 4 - a;
        sc[sp] = ch.x, sj[sp++] = a;
        for (int it = 0; it < 6 && sp > 0; ++it) {
            --sp;
            const int c = sc[sp], j = sj[sp];
            int s = (c < 0 || j < 2) ? 0 : (int)((word[c] >> (2 * (j - 2))) & 3u);
            if (s >= j) s = 0; /* (cannot happen: k_collapse_cost takes a < j) */
            if (s == 0) {
                if (nk < 4) kids[nk++] = c;
            } else if (sp + 2 <= 4) {
                const int2 cc = child[c];
                sc[sp] = cc.y, sj[sp++] = j - s;
                sc[sp] = cc.x, sj[sp++] = s;
            }
        }
    }
    const int stk = f.stack + (nk > 0 ? nk - 1 : 0);
    atomicMax(max_stack, (uint32_t)stk);
    /* as k_collapse: consecutive node indices for the inner children, consecutive record slots for
       the leaf children, one block each */
    uint32_t cnt[4] = {0u, 0u, 0u, 0u}; /* 0: an inner child; else the leaf's triangles */
    int n_in = 0;
    uint32_t n_leaf_tris = 0;
    for (int k = 0; k < nk; ++k) {
        const int c = kids[k];
        uint32_t m = 1;
        if (c >= 0 && n >= 2) {
            const uint32_t w = word[c];
            m = (w & kWordLeaf) ? (w >> 12) & 7u : 0u;
            if (m > kLeafMax) m = kLeafMax; /* (cannot happen: as_leaf implies size <= kLeafMax) */
        }
        cnt[k] = m;
        if (m) n_leaf_tris += m;
        else ++n_in;
    }
    const uint32_t node_base = n_in ? atomicAdd(n_nodes, (uint32_t)n_in) : 0u;
    const uint32_t tri_base = n_leaf_tris ? atomicAdd(n_tris_out, n_leaf_tris) : 0u;
    uint32_t next_node = node_base, next_tri = tri_base;
    float *nd = nodes4 + 32ull * f.out;
    for (int k = 0; k < 4; ++k) {
        int32_t code = RT_EMPTY_CHILD;
        float b[6] = {0, 0, 0, 0, 0, 0};
        if (k < nk) {
            const int c = kids[k];
            const uint32_t count = cnt[k];
            const float *src = (c >= 0 && n >= 2) ? nbox + 6ull * c : tbox + 6ull * perm[n >= 2 ? ~c : 0];
            for (int a = 0; a < 6; ++a) b[a] = src[a];
            if (count == 0) {
                const uint32_t id = next_node++;
                code = (int32_t)id;
                const uint32_t q = atomicAdd(n_next, 1u);
                next[q] = Frontier{c, (int)id, stk};
            } else {
                const uint32_t first = next_tri;
                next_tri += count;
                if (c >= 0 && n >= 2) {
                    /* count <= kLeafMax: at most 2 kLeafMax - 1 nodes, the stack never holds more
                       than kLeafMax of them */
                    int stack[kLeafMax + 1], sp = 0;
                    uint32_t q = 0;
                    stack[sp++] = c;
                    for (uint32_t it = 0; it < 2 * kLeafMax - 1 && sp > 0; ++it) {
                        const int x = stack[--sp];
                        if (x < 0) {
                            if (q < count) perm2[first + q++] = (uint32_t)(~x);
                        } else if (sp + 2 <= (int)kLeafMax + 1) {
                            stack[sp++] = child[x].y;
                            stack[sp++] = child[x].x;
                        }
                    }
                } else {
                    perm2[first] = n >= 2 ? (uint32_t)(~c) : 0u;
                }
                code = ~(int32_t)((first << 3) | (count - 1));
            }
        }
        nd[0 + k] = b[0];
        nd[4 + k] = b[3];
        nd[8 + k] = b[1];
        nd[12 + k] = b[4];
        nd[16 + k] = b[2];
        nd[20 + k] = b[5];
        nd[24 + k] = __int_as_float(code);
        nd[28 + k] = 0.0f;
    }
}

/* 6a. compressed nodes (rt_quant.h, the host builder's encoder); flag = 1 if any
   node cannot be encoded (the traversal then uses the full-precision nodes) */
__global__ void k_quantize(const float *__restrict__ nodes4, uint32_t n_nodes, uint32_t *__restrict__ q4,
                           uint32_t *__restrict__ fail)
{
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i >= n_nodes) return;
    if (!rt_quantize_node4(nodes4 + 32ull * i, q4 + (uint64_t)RT_QNODE_DWORDS * i)) atomicOr(fail, 1u);
}

/* 6b. triangle records in slot order: (v0, orig), (v1 - v0), (v2 - v0) (rtcommon.h:20-37) */
__global__ void k_tri_records(const float *__restrict__ verts, const int32_t *__restrict__ idx,
                              const uint32_t *__restrict__ perm, const uint32_t *__restrict__ perm2, uint32_t n,
                              float *__restrict__ tris)
{
    const uint32_t s = blockIdx.x * kB + threadIdx.x;
    if (s >= n) return;
    const uint32_t t = perm[perm2 ? perm2[s] : s]; /* (no perm2: the list's own order, the left-out tail) */
    const float *a = verts + 3ull * (uint32_t)idx[3ull * t];
    const float *p1 = verts + 3ull * (uint32_t)idx[3ull * t + 1];
    const float *p2 = verts + 3ull * (uint32_t)idx[3ull * t + 2];
    float *o = tris + 12ull * s;
    o[0] = a[0];
    o[1] = a[1];
    o[2] = a[2];
    o[3] = __int_as_float((int32_t)t);
    o[4] = p1[0] - a[0];
    o[5] = p1[1] - a[1];
    o[6] = p1[2] - a[2];
    o[7] = 0.0f;
    o[8] = p2[0] - a[0];
    o[9] = p2[1] - a[1];
    o[10] = p2[2] - a[2];
    o[11] = 0.0f;
}

/* 6c. normal boxes of the compressed nodes (rt_quant.h determinant cull), one level of the
   4-wide tree per launch from the deepest up: a node's inner children (the next level) are
   done, its leaf children's triangles are read from the records.  binary64, as the host
   builder. */
struct NBox {
    double lo[3], hi[3], err;
};
__global__ void k_nbox(const float *__restrict__ nodes4, uint32_t node_base, uint32_t first, uint32_t last,
                       const float *__restrict__ tris, NBox *__restrict__ nb, uint32_t *__restrict__ q4)
{
    /* nodes4 holds the nodes from node_base on (the shadow tree's, numbered after the first tree's) */
    const uint32_t i = first + blockIdx.x * kB + threadIdx.x;
    if (i >= last) return;
    NBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = __builtin_huge_val();
        b.hi[a] = -__builtin_huge_val();
    }
    b.err = 0.0;
    const float *f = nodes4 + 32ull * (i - node_base);
    for (int k = 0; k < 4; ++k) {
        const int32_t c = __float_as_int(f[24 + k]);
        if (c == RT_EMPTY_CHILD) continue;
        if (c >= 0) {
            const NBox &cb = nb[c];
            for (int a = 0; a < 3; ++a) {
                b.lo[a] = fmin(b.lo[a], cb.lo[a]);
                b.hi[a] = fmax(b.hi[a], cb.hi[a]);
            }
            b.err = fmax(b.err, cb.err);
            continue;
        }
        const int32_t enc = ~c, lf = enc >> 3, cnt = (enc & 7) + 1;
        for (int32_t j = 0; j < cnt; ++j) {
            const float *o = tris + 12ull * (uint32_t)(lf + j);
            const double e1[3] = {o[4], o[5], o[6]}, e2[3] = {o[8], o[9], o[10]};
            const double n[3] = {e2[1] * e1[2] - e2[2] * e1[1], e2[2] * e1[0] - e2[0] * e1[2],
                                 e2[0] * e1[1] - e2[1] * e1[0]};
            for (int a = 0; a < 3; ++a) {
                b.lo[a] = fmin(b.lo[a], n[a]);
                b.hi[a] = fmax(b.hi[a], n[a]);
            }
            b.err = fmax(b.err, (fabs(e1[0]) + fabs(e1[1]) + fabs(e1[2])) * (fabs(e2[0]) + fabs(e2[1]) + fabs(e2[2])));
        }
    }
    nb[i] = b;
    rt_qnode_set_nbox(q4 + (uint64_t)RT_QNODE_DWORDS * i, b.lo, b.hi, b.err);
}

/* ---- RT_BUILD_OPT_LIGHTS: what the host build does around its trees ---- */

/* 0a. one class byte per triangle by the rules of rt_tri_rules.h on the record's floats:
   2 left out (never_hit), 1 parked (kept, never_occludes for every light), 0 a possible occluder */
enum : uint8_t { kClsOccluder = 0, kClsParked = 1, kClsOut = 2 };
__global__ void k_classify(const float *__restrict__ verts, const int32_t *__restrict__ idx, uint32_t n, int cull,
                           const float *__restrict__ lights, uint32_t n_lights, uint8_t *__restrict__ cls)
{
    const uint32_t t = blockIdx.x * kB + threadIdx.x;
    if (t >= n) return;
    const float *a = verts + 3ull * (uint32_t)idx[3ull * t];
    const float *p1 = verts + 3ull * (uint32_t)idx[3ull * t + 1];
    const float *p2 = verts + 3ull * (uint32_t)idx[3ull * t + 2];
    const float A[3] = {a[0], a[1], a[2]};
    const float e1[3] = {p1[0] - A[0], p1[1] - A[1], p1[2] - A[2]};
    const float e2[3] = {p2[0] - A[0], p2[1] - A[1], p2[2] - A[2]};
    uint8_t c = kClsOccluder;
    if (cull && never_hit_edges(e1, e2)) c = kClsOut;
    else if (n_lights && never_occludes_edges(A, e1, e2, lights, n_lights)) c = kClsParked;
    cls[t] = c;
}

/* 0b. flags[t] = occluder << 32 | parked (without a split the parked count as occluders): one
   exclusive sum numbers both ranges, the left-out ones take what remains */
__global__ void k_class_flags(const uint8_t *__restrict__ cls, uint32_t n, int split, uint64_t *__restrict__ flags)
{
    const uint32_t t = blockIdx.x * kB + threadIdx.x;
    if (t >= n) return;
    const uint8_t c = cls[t];
    const bool parked = split && c == kClsParked;
    flags[t] = ((uint64_t)(c != kClsOut && !parked) << 32) | (uint64_t)parked;
}

/* 0c. the stable compaction to the three slot ranges, in triangle order: the occluders in
   [0, n0), the parked in [n0, n0 + n1), the left-out after them.  tot[0] = n0, tot[1] = n1. */
__global__ void k_class_totals(const uint64_t *__restrict__ flags, const uint64_t *__restrict__ scan, uint32_t n,
                               uint32_t *__restrict__ tot)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t s = scan[n - 1] + flags[n - 1];
    tot[0] = (uint32_t)(s >> 32);
    tot[1] = (uint32_t)s;
}
__global__ void k_class_scatter(const uint64_t *__restrict__ flags, const uint64_t *__restrict__ scan, uint32_t n,
                                uint32_t n0, uint32_t n1, uint32_t *__restrict__ order)
{
    const uint32_t t = blockIdx.x * kB + threadIdx.x;
    if (t >= n) return;
    const uint64_t fl = flags[t], sc = scan[t];
    const uint32_t s0 = (uint32_t)(sc >> 32), s1 = (uint32_t)sc;
    uint32_t pos;
    if (fl >> 32) pos = s0;
    else if (fl & 1u) pos = n0 + s1;
    else pos = n0 + n1 + (t - s0 - s1);
    if (pos < n) order[pos] = t;
}

/* 5'. the shadow tree's root (node 0 of its array): exactly two children, A (node 1) then B
   (node 2), each the root of its own binary tree */
__global__ void k_cone_root(const float *__restrict__ box_a, const float *__restrict__ box_b, float *__restrict__ nd)
{
    const int k = threadIdx.x;
    if (blockIdx.x || k >= 4) return;
    const float *b = k == 0 ? box_a : box_b;
    const bool used = k < 2;
    nd[0 + k] = used ? b[0] : 0.0f;
    nd[4 + k] = used ? b[3] : 0.0f;
    nd[8 + k] = used ? b[1] : 0.0f;
    nd[12 + k] = used ? b[4] : 0.0f;
    nd[16 + k] = used ? b[2] : 0.0f;
    nd[20 + k] = used ? b[5] : 0.0f;
    nd[24 + k] = __int_as_float(used ? k + 1 : RT_EMPTY_CHILD);
    nd[28 + k] = 0.0f;
}

/* 5''. the shadow tree's links in the numbering of both trees: its nodes follow the first
   tree's n_a, its records the first tree's n_tris (rt_mesh.cpp, the host build's layout) */
__global__ void k_shadow_links(float *__restrict__ nodes4, uint32_t n_nodes, uint32_t n_a, uint32_t n_tris)
{
    const uint32_t j = blockIdx.x * kB + threadIdx.x;
    if (j >= 4u * n_nodes) return;
    float *w = nodes4 + 32ull * (j >> 2) + 24 + (j & 3u);
    int32_t code = __float_as_int(*w);
    if (code == RT_EMPTY_CHILD) return;
    if (code >= 0) {
        code += (int32_t)n_a;
    } else {
        const uint32_t enc = (uint32_t)(~code);
        code = ~(int32_t)((((enc >> 3) + n_tris) << 3) | (enc & 7u));
    }
    *w = __int_as_float(code);
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kB - 1) / kB); }

/* RAII scratch */
struct DevBuf {
    void *p = nullptr;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
};

} // namespace

#define GCHK(x)                                                                                                        \
    do {                                                                                                               \
        const hipError_t e_ = (x);                                                                                     \
        if (e_ != hipSuccess) {                                                                                        \
            err = std::string(#x) + ": " + hipGetErrorString(e_);                                                      \
            return (int)e_;                                                                                            \
        }                                                                                                              \
    } while (0)

namespace {
/* Stage times of one build by HIP events, for profiles/ploc/measure.py: with RT_BUILD_PROFILE
   naming a file, every build appends one JSON line to it.  Without it nothing is recorded and
   nothing waits. */
struct BuildProfile {
    bool on = false, ploc = false;
    const char *path = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::vector<std::pair<std::string, float>> ms;
    explicit BuildProfile(bool ploc_) : ploc(ploc_)
    {
        path = getenv("RT_BUILD_PROFILE");
        on = path && *path && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    }
    ~BuildProfile()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void begin(hipStream_t st)
    {
        if (on) (void)hipEventRecord(ev[0], st);
    }
    /* the time since begin() or the last lap(), added to `name` */
    void lap(hipStream_t st, const char *name)
    {
        if (!on) return;
        float t = 0.0f;
        (void)hipEventRecord(ev[1], st);
        (void)hipEventSynchronize(ev[1]);
        (void)hipEventElapsedTime(&t, ev[0], ev[1]);
        for (auto &m : ms)
            if (m.first == name) {
                m.second += t;
                t = -1.0f;
                break;
            }
        if (t >= 0.0f) ms.emplace_back(name, t);
        (void)hipEventRecord(ev[0], st);
    }
    void write(uint32_t n_tris, uint32_t rounds, double seconds) const
    {
        if (!on) return;
        FILE *f = fopen(path, "a");
        if (!f) return;
        fprintf(f, "{\"builder\": \"%s\", \"n_tris\": %u, \"rounds\": %u, \"build_seconds\": %.6f, \"ms\": {",
                ploc ? "ploc" : "gpu", n_tris, rounds, seconds);
        for (size_t i = 0; i < ms.size(); ++i) fprintf(f, "%s\"%s\": %.4f", i ? ", " : "", ms[i].first.c_str(), ms[i].second);
        fprintf(f, "}}\n");
        fclose(f);
    }
};
} // namespace

/* The PLOC rounds (k_ploc_*): child / nbox / nsize of the n - 1 binary nodes, the root last
   (node n - 2).  Rounds search until `cap`, then halve (nn = i ^ 1), so the count is bounded
   whatever the boxes are; the cluster count is read back once per round. */
static int ploc_tree(const float *tbox, const uint32_t *perm, int n, int2 *child, float *nbox, uint32_t *nsize,
                     hipStream_t st, BuildProfile &prof, uint32_t &rounds, std::string &err)
{
    DevBuf d_cid[2], d_cbox[2], d_nn, d_flags, d_scan, d_tmp, d_c;
    for (int k = 0; k < 2; ++k) {
        GCHK(hipMalloc(&d_cid[k].p, 4ull * n));
        GCHK(hipMalloc(&d_cbox[k].p, 24ull * n));
    }
    GCHK(hipMalloc(&d_nn.p, 4ull * n));
    GCHK(hipMalloc(&d_flags.p, 8ull * n));
    GCHK(hipMalloc(&d_scan.p, 8ull * n));
    GCHK(hipMalloc(&d_c.p, sizeof(uint32_t)));
    size_t tmp_bytes = 0;
    GCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const uint64_t *)d_flags.p, (uint64_t *)d_scan.p, n, st));
    GCHK(hipMalloc(&d_tmp.p, tmp_bytes ? tmp_bytes : 1));
    hipLaunchKernelGGL(k_ploc_init, dim3(blocks_for(n)), dim3(kB), 0, st, tbox, perm, n, (int *)d_cid[0].p,
                       (float *)d_cbox[0].p);
    GCHK(hipGetLastError());
    prof.lap(st, "ploc_init");
    int log2n = 0;
    while ((1ll << log2n) < n) ++log2n;
    const uint32_t cap = 6u * log2n + 16u, bound = cap + log2n;
    int C = n, K = 0, cur = 0;
    for (rounds = 0; C > 1; ++rounds) {
        if (rounds >= bound) {
            err = "PLOC build: round bound passed";
            return -1;
        }
        const unsigned g = blocks_for(C);
        hipLaunchKernelGGL(k_ploc_nn, dim3(g), dim3(kB), 0, st, (const float *)d_cbox[cur].p, C,
                           rounds >= cap ? 1 : 0, (int *)d_nn.p);
        GCHK(hipGetLastError());
        prof.lap(st, "ploc_nn");
        hipLaunchKernelGGL(k_ploc_flags, dim3(g), dim3(kB), 0, st, (const int *)d_nn.p, C, (uint64_t *)d_flags.p);
        GCHK(hipGetLastError());
        prof.lap(st, "ploc_flags");
        size_t tb = tmp_bytes;
        GCHK(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tb, (const uint64_t *)d_flags.p, (uint64_t *)d_scan.p, C, st));
        prof.lap(st, "ploc_scan");
        hipLaunchKernelGGL(k_ploc_merge, dim3(g), dim3(kB), 0, st, (const int *)d_cid[cur].p,
                           (const float *)d_cbox[cur].p, (const int *)d_nn.p, (const uint64_t *)d_flags.p,
                           (const uint64_t *)d_scan.p, C, K, n - 1, (int *)d_cid[1 - cur].p, (float *)d_cbox[1 - cur].p,
                           child, nbox, nsize, (uint32_t *)d_c.p);
        GCHK(hipGetLastError());
        uint32_t c_new = 0;
        GCHK(hipMemcpyAsync(&c_new, d_c.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        GCHK(hipStreamSynchronize(st));
        prof.lap(st, "ploc_merge");
        if (c_new < 1 || c_new >= (uint32_t)C) {
            err = "PLOC build: no progress";
            return -1;
        }
        K += C - (int)c_new;
        C = (int)c_new;
        cur = 1 - cur;
    }
    if (K != n - 1) {
        err = "PLOC build: node count";
        return -1;
    }
    return 0;
}


namespace {

/* Steps 1-4 (or 3'-4') over the m triangles a list names (sub; nullptr: triangles 0 .. m - 1):
   the sorted order (perm: slot -> triangle) and the binary tree, everything the collapse reads.
   tbox / cent are per triangle of the mesh, written here for the list's. */
struct BinTree {
    DevBuf bounds, keys, keys2, vals, perm, tmp, child, range, pin, pleaf, nbox, flags, nsize;
    DevBuf cost, word, cflags; /* RT_COLLAPSE_SAH: k_collapse_cost's D, words and arrival flags */
    int m = 0, root = 0; /* root: the binary root (~0: the single triangle of m == 1) */
};

int build_binary(const float *verts, const int32_t *idx, const uint32_t *sub, int m, float *tbox, float *cent,
                 bool ploc, hipStream_t st, BuildProfile &prof, uint32_t &rounds, BinTree &T, std::string &err)
{
    T.m = m;
    GCHK(hipMalloc(&T.bounds.p, 6 * sizeof(uint32_t)));
    const uint32_t init_bounds[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    GCHK(hipMemcpyAsync(T.bounds.p, init_bounds, sizeof(init_bounds), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_prep, dim3(blocks_for(m)), dim3(kB), 0, st, verts, idx, sub, (uint32_t)m, tbox, cent,
                       (uint32_t *)T.bounds.p);
    GCHK(hipGetLastError());

    GCHK(hipMalloc(&T.keys.p, 8ull * m));
    GCHK(hipMalloc(&T.keys2.p, 8ull * m));
    GCHK(hipMalloc(&T.vals.p, 4ull * m));
    GCHK(hipMalloc(&T.perm.p, 4ull * m));
    hipLaunchKernelGGL(k_morton, dim3(blocks_for(m)), dim3(kB), 0, st, (const float *)cent, sub, (uint32_t)m,
                       (const uint32_t *)T.bounds.p, (uint64_t *)T.keys.p, (uint32_t *)T.vals.p);
    GCHK(hipGetLastError());
    size_t tmp_bytes = 0;
    GCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (uint64_t *)T.keys.p, (uint64_t *)T.keys2.p,
                                            (uint32_t *)T.vals.p, (uint32_t *)T.perm.p, m, 0, 63, st));
    GCHK(hipMalloc(&T.tmp.p, tmp_bytes));
    GCHK(hipcub::DeviceRadixSort::SortPairs(T.tmp.p, tmp_bytes, (uint64_t *)T.keys.p, (uint64_t *)T.keys2.p,
                                            (uint32_t *)T.vals.p, (uint32_t *)T.perm.p, m, 0, 63, st));

    prof.lap(st, "sort");
    const uint64_t n_inner = m >= 2 ? (uint64_t)m - 1 : 1;
    GCHK(hipMalloc(&T.child.p, 8ull * n_inner));
    GCHK(hipMalloc(&T.nbox.p, 24ull * n_inner));
    T.root = m >= 2 ? 0 : ~0;
    if (ploc) {
        GCHK(hipMalloc(&T.nsize.p, 4ull * n_inner));
        if (m >= 2) {
            const int e = ploc_tree((const float *)tbox, (const uint32_t *)T.perm.p, m, (int2 *)T.child.p,
                                    (float *)T.nbox.p, (uint32_t *)T.nsize.p, st, prof, rounds, err);
            if (e) return e;
            T.root = m - 2;
        }
    } else {
        GCHK(hipMalloc(&T.range.p, 8ull * n_inner));
        GCHK(hipMalloc(&T.pin.p, 4ull * n_inner));
        GCHK(hipMalloc(&T.pleaf.p, 4ull * m));
        GCHK(hipMalloc(&T.flags.p, 4ull * n_inner));
        GCHK(hipMemsetAsync(T.flags.p, 0, 4ull * n_inner, st));
        GCHK(hipMemsetAsync(T.pin.p, 0xFF, 4ull * n_inner, st));
        if (m >= 2) {
            hipLaunchKernelGGL(k_radix_tree, dim3(blocks_for(m - 1)), dim3(kB), 0, st, (const uint64_t *)T.keys2.p, m,
                               (int2 *)T.child.p, (int2 *)T.range.p, (int *)T.pin.p, (int *)T.pleaf.p);
            GCHK(hipGetLastError());
            hipLaunchKernelGGL(k_boxes, dim3(blocks_for(m)), dim3(kB), 0, st, (const float *)tbox,
                               (const uint32_t *)T.perm.p, m, (const int2 *)T.child.p, (const int *)T.pin.p,
                               (const int *)T.pleaf.p, (float *)T.nbox.p, (int *)T.flags.p);
            GCHK(hipGetLastError());
        }
    }
    prof.lap(st, "tree");
    return 0;
}

/* Step 5 over one binary tree (its root becomes node 0), or over the cone split's two: A's root
   is node 1 and B's node 2 under the root k_cone_root wrote, the nodes of both are handed out
   from one counter, and every level is one launch for A's frontier and then one for B's, so a
   level of the whole tree is an index range in which A's nodes come before B's (what
   rt_mesh.cpp's tree_levels and the refit read off the links).  A part's leaves take record
   slots from its own counter, from tri_base[p] on.
   cnt, 16 words: [2] nodes, [3] max stack, [5] the quantisation failure flag (k_quantize);
   per part p at 8 p: [0] [1] its two frontiers' sizes, [4] record slots handed out.
   d_front: the parts' frontier buffers, the caller's (freed with the build's other scratch, after
   build_seconds is taken, as before). */
struct Collapsed {
    uint32_t n_nodes = 0, depth = 0, stack = 0;
    uint32_t tri_end[2] = {0u, 0u};
    std::vector<uint32_t> level_end; /* node ids of level L: [level_end[L-1], level_end[L]) */
};

int collapse(BinTree *const *parts, int n_parts, const uint32_t *tri_base, bool ploc, bool sah, const float *tbox,
             float *nodes4, uint32_t *perm2, uint32_t *cnt, DevBuf (*d_front)[2], hipStream_t st, BuildProfile &prof,
             Collapsed &out, std::string &err)
{
    const bool two = n_parts == 2;
    /* RT_COLLAPSE_SAH: the bottom-up pass over every part, each on its own */
    for (int p = 0; sah && p < n_parts; ++p) {
        BinTree &T = *parts[p];
        if (T.m < 2) continue;
        const uint64_t n_inner = (uint64_t)T.m - 1;
        GCHK(hipMalloc(&T.cost.p, 16ull * n_inner));
        GCHK(hipMalloc(&T.word.p, 4ull * n_inner));
        GCHK(hipMalloc(&T.cflags.p, 4ull * n_inner));
        GCHK(hipMemsetAsync(T.cflags.p, 0, 4ull * n_inner, st));
        if (ploc) { /* the PLOC tree has no parent links yet */
            GCHK(hipMalloc(&T.pin.p, 4ull * n_inner));
            GCHK(hipMalloc(&T.pleaf.p, 4ull * T.m));
            GCHK(hipMemsetAsync(T.pin.p, 0xFF, 4ull * n_inner, st));
            hipLaunchKernelGGL(k_parents, dim3(blocks_for(n_inner)), dim3(kB), 0, st, (const int2 *)T.child.p,
                               (int)n_inner, (int *)T.pin.p, (int *)T.pleaf.p);
            GCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_collapse_cost, dim3(blocks_for(T.m)), dim3(kB), 0, st, tbox, (const uint32_t *)T.perm.p, T.m,
                           (const int2 *)T.child.p, (const int2 *)T.range.p, (const uint32_t *)T.nsize.p,
                           (const int *)T.pin.p, (const int *)T.pleaf.p, (const float *)T.nbox.p, (int *)T.cflags.p,
                           (float *)T.cost.p, (uint32_t *)T.word.p);
        GCHK(hipGetLastError());
    }
    if (sah) prof.lap(st, "collapse_cost");
    uint32_t init_counts[16] = {0u};
    init_counts[2] = two ? 3u : 1u;
    init_counts[3] = two ? 1u : 0u; /* the root's other child waits on the stack */
    for (int p = 0; p < n_parts; ++p) {
        const uint64_t cap4 = (parts[p]->m >= 2 ? (uint64_t)parts[p]->m - 1 : 1) + 1;
        GCHK(hipMalloc(&d_front[p][0].p, sizeof(Frontier) * cap4));
        GCHK(hipMalloc(&d_front[p][1].p, sizeof(Frontier) * cap4));
        const Frontier root = {parts[p]->root, two ? p + 1 : 0, two ? 1 : 0};
        GCHK(hipMemcpyAsync(d_front[p][0].p, &root, sizeof(root), hipMemcpyHostToDevice, st));
        init_counts[8 * p + 0] = 1u;
        init_counts[8 * p + 4] = tri_base[p];
    }
    GCHK(hipMemcpyAsync(cnt, init_counts, sizeof(init_counts), hipMemcpyHostToDevice, st));
    uint32_t level_size[2] = {1u, two ? 1u : 0u}, depth = 0;
    int cur = 0;
    out.level_end.assign(1, 1u);
    if (two) out.level_end.push_back(3u);
    while (level_size[0] > 0 || level_size[1] > 0) {
        ++depth;
        uint32_t n_alloc = 0;
        for (int p = 0; p < n_parts; ++p) {
            if (!level_size[p]) continue;
            const BinTree &T = *parts[p];
            uint32_t *c = cnt + 8 * p;
            GCHK(hipMemsetAsync(c + (1 - cur), 0, sizeof(uint32_t), st));
            if (sah)
                hipLaunchKernelGGL(k_collapse_sah, dim3(blocks_for(level_size[p])), dim3(kB), 0, st,
                                   (const Frontier *)d_front[p][cur].p, c + cur, (Frontier *)d_front[p][1 - cur].p,
                                   c + (1 - cur), cnt + 2, cnt + 3, (const int2 *)T.child.p, (const uint32_t *)T.word.p,
                                   (const float *)T.nbox.p, tbox, (const uint32_t *)T.perm.p, T.m, nodes4, c + 4, perm2);
            else
            hipLaunchKernelGGL(ploc ? k_collapse<true> : k_collapse<false>, dim3(blocks_for(level_size[p])), dim3(kB), 0,
                               st, (const Frontier *)d_front[p][cur].p, c + cur, (Frontier *)d_front[p][1 - cur].p,
                               c + (1 - cur), cnt + 2, cnt + 3, (const int2 *)T.child.p, (const int2 *)T.range.p,
                               (const uint32_t *)T.nsize.p, (const float *)T.nbox.p, tbox, (const uint32_t *)T.perm.p,
                               T.m, nodes4, c + 4, perm2);
            GCHK(hipGetLastError());
            GCHK(hipMemcpyAsync(&level_size[p], c + (1 - cur), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        GCHK(hipMemcpyAsync(&n_alloc, cnt + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        GCHK(hipStreamSynchronize(st));
        if (level_size[0] > 0 || level_size[1] > 0) out.level_end.push_back(n_alloc);
        cur = 1 - cur;
        if (depth > 4096) {
            err = "GPU BVH collapse did not terminate";
            return -1;
        }
    }
    uint32_t counts[16];
    GCHK(hipMemcpyAsync(counts, cnt, sizeof(counts), hipMemcpyDeviceToHost, st));
    GCHK(hipStreamSynchronize(st));
    out.n_nodes = counts[2];
    out.depth = depth;
    out.stack = counts[3];
    for (int p = 0; p < n_parts; ++p) out.tri_end[p] = counts[8 * p + 4];
    return 0;
}

/* Step 6c for the nodes [base, base + n_nodes) whose full-precision form is nodes4 */
int nbox_levels(const float *nodes4, uint32_t base, const std::vector<uint32_t> &level_end, const float *tris, NBox *nb,
                uint32_t *q4, hipStream_t st, std::string &err)
{
    for (size_t L = level_end.size(); L-- > 0;) {
        const uint32_t a = base + (L ? level_end[L - 1] : 0u), b = base + level_end[L];
        if (b <= a) continue;
        hipLaunchKernelGGL(k_nbox, dim3(blocks_for(b - a)), dim3(kB), 0, st, nodes4, base, a, b, tris, nb, q4);
        GCHK(hipGetLastError());
    }
    return 0;
}

} // namespace

int rt_build_bvh_gpu(const float *verts_h, uint32_t n_verts, const int32_t *idx_h, uint32_t n_tris, RtGpuBvh &out,
                     std::string &err, void *stream, bool det_cull, bool ploc, const RtGpuBuildLights *lights, bool sah)
{
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = (hipStream_t)stream;
    DevBuf d_verts, d_idx, d_tbox, d_cent, d_counts, d_perm2, d_cls, d_cflags, d_cscan, d_ctmp, d_order, d_tot,
        d_lights, d_nodes4s, d_perm2s, d_front[1][2], d_front_s[2][2];
    BuildProfile prof(ploc);
    prof.begin(st);
    GCHK(hipMalloc(&d_verts.p, 12ull * n_verts));
    GCHK(hipMalloc(&d_idx.p, 12ull * n_tris));
    GCHK(hipMemcpyAsync(d_verts.p, verts_h, 12ull * n_verts, hipMemcpyHostToDevice, st));
    GCHK(hipMemcpyAsync(d_idx.p, idx_h, 12ull * n_tris, hipMemcpyHostToDevice, st));
    GCHK(hipMalloc(&d_tbox.p, 24ull * n_tris));
    GCHK(hipMalloc(&d_cent.p, 12ull * n_tris));
    const float *verts = (const float *)d_verts.p;
    const int32_t *idx = (const int32_t *)d_idx.p;

    /* RT_BUILD_OPT_LIGHTS: the classes, and the triangles in class order (d_order): the possible
       occluders [0, n0), the parked [n0, n_hit), the left-out after them */
    const bool opt = lights && lights->cull;
    uint32_t n_hit = n_tris, n0 = 0, n1 = 0;
    bool split = false;
    if (opt) {
        const uint32_t n_lights = lights->lights ? lights->n_lights : 0u;
        if (n_lights) {
            GCHK(hipMalloc(&d_lights.p, 16ull * n_lights));
            GCHK(hipMemcpyAsync(d_lights.p, lights->lights, 16ull * n_lights, hipMemcpyHostToDevice, st));
        }
        GCHK(hipMalloc(&d_cls.p, n_tris));
        GCHK(hipMalloc(&d_cflags.p, 8ull * n_tris));
        GCHK(hipMalloc(&d_cscan.p, 8ull * n_tris));
        GCHK(hipMalloc(&d_order.p, 4ull * n_tris));
        GCHK(hipMalloc(&d_tot.p, 2 * sizeof(uint32_t)));
        size_t tmp_bytes = 0;
        GCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const uint64_t *)d_cflags.p, (uint64_t *)d_cscan.p,
                                              (int)n_tris, st));
        GCHK(hipMalloc(&d_ctmp.p, tmp_bytes ? tmp_bytes : 1));
        hipLaunchKernelGGL(k_classify, dim3(blocks_for(n_tris)), dim3(kB), 0, st, verts, idx, n_tris, 1,
                           (const float *)d_lights.p, n_lights, (uint8_t *)d_cls.p);
        GCHK(hipGetLastError());
        uint32_t tot[2] = {0u, 0u};
        auto number = [&](int with_split) -> int { /* flags, their sum, the totals */
            hipLaunchKernelGGL(k_class_flags, dim3(blocks_for(n_tris)), dim3(kB), 0, st, (const uint8_t *)d_cls.p,
                               n_tris, with_split, (uint64_t *)d_cflags.p);
            GCHK(hipGetLastError());
            size_t tb = tmp_bytes;
            GCHK(hipcub::DeviceScan::ExclusiveSum(d_ctmp.p, tb, (const uint64_t *)d_cflags.p, (uint64_t *)d_cscan.p,
                                                  (int)n_tris, st));
            hipLaunchKernelGGL(k_class_totals, dim3(1), dim3(64), 0, st, (const uint64_t *)d_cflags.p,
                               (const uint64_t *)d_cscan.p, n_tris, (uint32_t *)d_tot.p);
            GCHK(hipGetLastError());
            GCHK(hipMemcpyAsync(tot, d_tot.p, sizeof(tot), hipMemcpyDeviceToHost, st));
            GCHK(hipStreamSynchronize(st));
            return 0;
        };
        if (int e = number(1)) return e;
        if (tot[0] + tot[1] == 0) { /* nothing hittable: triangle 0 stays, the tree is never empty */
            GCHK(hipMemsetAsync(d_cls.p, kClsOccluder, 1, st));
            if (int e = number(1)) return e;
        }
        /* the host build's conditions for the split (rt_bvh.cpp, rt_mesh.cpp) */
        split = n_lights > 0 && tot[0] > kLeafMax && tot[1] > kLeafMax && 2ull * n_tris < (1ull << 28);
        if (!split && tot[1])
            if (int e = number(0)) return e;
        n0 = tot[0];
        n1 = tot[1];
        n_hit = n0 + n1;
        if (n_hit < 1 || n_hit > n_tris) {
            err = "GPU BVH build: class counts";
            return -1;
        }
        hipLaunchKernelGGL(k_class_scatter, dim3(blocks_for(n_tris)), dim3(kB), 0, st, (const uint64_t *)d_cflags.p,
                           (const uint64_t *)d_cscan.p, n_tris, n0, n1, (uint32_t *)d_order.p);
        GCHK(hipGetLastError());
        prof.lap(st, "classify");
    }
    const uint32_t *order = (const uint32_t *)d_order.p;

    BinTree all;
    if (int e = build_binary(verts, idx, order, (int)n_hit, (float *)d_tbox.p, (float *)d_cent.p, ploc, st, prof,
                             out.rounds, all, err))
        return e;

    /* collapse: the 4-wide tree has fewer nodes than the binary tree has inner nodes */
    const uint64_t cap4 = (n_hit >= 2 ? (uint64_t)n_hit - 1 : 1) + 1;
    float *nodes4 = nullptr;
    GCHK(hipMalloc(&nodes4, 128ull * cap4));
    out.nodes4 = nodes4;
    GCHK(hipMalloc(&d_counts.p, 16 * sizeof(uint32_t)));
    GCHK(hipMalloc(&d_perm2.p, 4ull * n_hit));
    uint32_t *cnt = (uint32_t *)d_counts.p;
    Collapsed ca, cs;
    {
        BinTree *parts[1] = {&all};
        const uint32_t base[1] = {0u};
        if (int e = collapse(parts, 1, base, ploc, sah, (const float *)d_tbox.p, nodes4, (uint32_t *)d_perm2.p, cnt,
                             d_front, st, prof, ca, err))
            return e;
    }
    prof.lap(st, "collapse");
    out.n_nodes4 = ca.n_nodes;
    out.depth4 = ca.depth;
    out.stack4 = out.stack4_all = ca.stack;
    out.n_hit = n_hit;
    if (ca.tri_end[0] != n_hit) {
        err = "GPU BVH collapse lost triangles";
        return -1;
    }

    /* the shadow queries' tree: A over the possible occluders, B over the parked, each built
       as the first tree was over its own slots, never merged across */
    BinTree ta, tb;
    if (split) {
        uint32_t rounds = 0;
        if (int e = build_binary(verts, idx, order, (int)n0, (float *)d_tbox.p, (float *)d_cent.p, ploc, st, prof, rounds,
                                 ta, err))
            return e;
        if (int e = build_binary(verts, idx, order + n0, (int)n1, (float *)d_tbox.p, (float *)d_cent.p, ploc, st, prof,
                                 rounds, tb, err))
            return e;
        GCHK(hipMalloc(&d_nodes4s.p, 128ull * ((uint64_t)n0 + n1 + 1)));
        GCHK(hipMalloc(&d_perm2s.p, 4ull * n_hit));
        hipLaunchKernelGGL(k_cone_root, dim3(1), dim3(64), 0, st, (const float *)ta.nbox.p + 6ull * ta.root,
                           (const float *)tb.nbox.p + 6ull * tb.root, (float *)d_nodes4s.p);
        GCHK(hipGetLastError());
        BinTree *parts[2] = {&ta, &tb};
        const uint32_t base[2] = {0u, n0};
        if (int e = collapse(parts, 2, base, ploc, sah, (const float *)d_tbox.p, (float *)d_nodes4s.p,
                             (uint32_t *)d_perm2s.p, cnt, d_front_s, st, prof, cs, err))
            return e;
        prof.lap(st, "collapse");
        if (cs.tri_end[0] != n0 || cs.tri_end[1] != n_hit) {
            err = "GPU BVH collapse lost triangles (shadow tree)";
            return -1;
        }
        hipLaunchKernelGGL(k_shadow_links, dim3(blocks_for(4ull * cs.n_nodes)), dim3(kB), 0, st, (float *)d_nodes4s.p,
                           cs.n_nodes, out.n_nodes4, n_tris);
        GCHK(hipGetLastError());
        out.n_nodes4_shadow = cs.n_nodes;
        out.n_cone = n0;
        out.stack4_all = std::max(ca.stack, cs.stack);
    }
    const uint32_t n_a = out.n_nodes4, n_s = out.n_nodes4_shadow;

    uint32_t *q4 = nullptr;
    GCHK(hipMalloc(&q4, 4ull * RT_QNODE_DWORDS * ((uint64_t)n_a + n_s)));
    out.nodes4q = q4;
    GCHK(hipMemsetAsync(cnt + 5, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_quantize, dim3(blocks_for(n_a)), dim3(kB), 0, st, (const float *)nodes4, n_a, q4, cnt + 5);
    GCHK(hipGetLastError());
    float *tris = nullptr;
    GCHK(hipMalloc(&tris, 48ull * n_tris * (split ? 2u : 1u)));
    out.tris = tris;
    hipLaunchKernelGGL(k_tri_records, dim3(blocks_for(n_hit)), dim3(kB), 0, st, verts, idx, (const uint32_t *)all.perm.p,
                       (const uint32_t *)d_perm2.p, n_hit, tris);
    GCHK(hipGetLastError());
    if (n_hit < n_tris) { /* the left-out triangles' records, in triangle order, for the linear traversal */
        hipLaunchKernelGGL(k_tri_records, dim3(blocks_for(n_tris - n_hit)), dim3(kB), 0, st, verts, idx, order + n_hit,
                           (const uint32_t *)nullptr, n_tris - n_hit, tris + 12ull * n_hit);
        GCHK(hipGetLastError());
    }
    if (split) {
        float *ts = tris + 12ull * n_tris;
        const uint32_t *p2 = (const uint32_t *)d_perm2s.p;
        hipLaunchKernelGGL(k_quantize, dim3(blocks_for(n_s)), dim3(kB), 0, st, (const float *)d_nodes4s.p, n_s,
                           q4 + (uint64_t)RT_QNODE_DWORDS * n_a, cnt + 5);
        GCHK(hipGetLastError());
        hipLaunchKernelGGL(k_tri_records, dim3(blocks_for(n0)), dim3(kB), 0, st, verts, idx, (const uint32_t *)ta.perm.p,
                           p2, n0, ts);
        GCHK(hipGetLastError());
        hipLaunchKernelGGL(k_tri_records, dim3(blocks_for(n1)), dim3(kB), 0, st, verts, idx, (const uint32_t *)tb.perm.p,
                           p2 + n0, n1, ts + 12ull * n0);
        GCHK(hipGetLastError());
        if (n_hit < n_tris) {
            hipLaunchKernelGGL(k_tri_records, dim3(blocks_for(n_tris - n_hit)), dim3(kB), 0, st, verts, idx,
                               order + n_hit, (const uint32_t *)nullptr, n_tris - n_hit, ts + 12ull * n_hit);
            GCHK(hipGetLastError());
        }
    }
    if (det_cull) {
        DevBuf d_nb;
        GCHK(hipMalloc(&d_nb.p, sizeof(NBox) * ((uint64_t)n_a + n_s)));
        if (int e = nbox_levels(nodes4, 0u, ca.level_end, tris, (NBox *)d_nb.p, q4, st, err)) return e;
        if (split)
            if (int e = nbox_levels((const float *)d_nodes4s.p, n_a, cs.level_end, tris, (NBox *)d_nb.p, q4, st, err))
                return e;
        GCHK(hipStreamSynchronize(st));
    }
    uint32_t qfail = 0;
    GCHK(hipMemcpyAsync(&qfail, cnt + 5, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GCHK(hipStreamSynchronize(st));
    if (qfail && split) {
        /* the shadow tree lives in compressed nodes alone: without them the build without the split */
        (void)hipFree(nodes4);
        (void)hipFree(q4);
        (void)hipFree(tris);
        out = RtGpuBvh();
        RtGpuBuildLights plain = *lights;
        plain.n_lights = 0;
        const int e = rt_build_bvh_gpu(verts_h, n_verts, idx_h, n_tris, out, err, stream, det_cull, ploc, &plain, sah);
        out.build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return e;
    }
    if (qfail) { /* not encodable: full-precision nodes only */
        (void)hipFree(q4);
        out.nodes4q = nullptr;
    }
    prof.lap(st, "records");
    out.build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    prof.write(n_tris, out.rounds, out.build_seconds);
    return 0;
}
