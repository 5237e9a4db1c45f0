/*
 * rt_refit.hip — new vertex positions for the mesh of the last rt_set_mesh, without a build:
 * the records, the boxes, the compressed planes and the normal boxes of both trees recomputed
 * on the device from the trees' own links and record order (rt_update_mesh).
 *
 * What makes a refit exact: both builders number a 4-wide tree breadth-first (children above
 * their parents, a level an index range), every child box is the float min / max union of the
 * padded float32 boxes of the triangles below it (the pad of rt_bvh.cpp and k_prep), and the
 * encoders of rt_quant.h depend only on the full-precision node and the records.  So
 *
 *   k_refit_check    looks before anything is written: finite coordinates, the triangles the
 *                    builder left out still never_hit (rt_bvh.cpp's binary64 expression,
 *                    rt_tri_rules.h), and the bounds of the referenced vertices;
 *   k_refit_records  rewrites every record slot of both trees' halves and the slot's padded box;
 *   k_refit_levels   rewrites the nodes, deepest level first: the full-precision node (the
 *                    closest-hit tree's in place, the shadow tree's in a workspace: the device
 *                    keeps that tree compressed only), rt_quantize_node4, the normal box;
 *   k_refit_area     sums the closest-hit tree's child half-areas (the quality signal);
 *   k_refit_cone     (a device build's cone split) asks whether every parked
 *                    triangle still never occludes the lights the split was made for.
 *
 * The traversal and k_tris are not touched: a refitted tree is a tree check_tree accepts.
 */
#include <hip/hip_runtime.h>

#include <cmath>

#include "rt_internal.h"
#include "rt_quant.h"
#include "rt_tri_rules.h"

#pragma clang fp contract(off)

namespace {

constexpr int kB = 256;

__device__ __forceinline__ uint32_t f2key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

/* per-wave sum of a small count, one atomic per wave */
__device__ __forceinline__ void wave_add(uint32_t *dst, uint32_t v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

/* res: RT_REFIT_RES_* words.  Writes nothing else. */
__global__ void k_refit_check(const float *__restrict__ verts, uint32_t n_verts, const int32_t *__restrict__ idx,
                              uint32_t n_tris, const float *__restrict__ tris, uint32_t n_hit,
                              uint32_t *__restrict__ res)
{
    const uint32_t stride = gridDim.x * kB, t0 = blockIdx.x * kB + threadIdx.x;
    uint32_t bad = 0, newly = 0;
    for (uint64_t i = t0; i < 3ull * n_verts; i += stride) {
        const float x = verts[i];
        if (!isfinite(x) || fabsf(x) > 1e15f) bad = 1; /* rt_validate_mesh's rule */
    }
    /* the culled tail of the closest-hit tree's half: the triangles left out of both trees */
    for (uint32_t s = n_hit + t0; s < n_tris; s += stride) {
        const uint32_t t = __float_as_uint(tris[12ull * s + 3]);
        if (t >= n_tris) {
            bad = 2;
            continue;
        }
        const float *a = verts + 3ull * (uint32_t)idx[3ull * t];
        const float *p1 = verts + 3ull * (uint32_t)idx[3ull * t + 1];
        const float *p2 = verts + 3ull * (uint32_t)idx[3ull * t + 2];
        if (!never_hit(a, p1, p2)) ++newly;
    }
    /* bounds of the vertices the triangles use (rt_mesh.cpp mesh_bounds) */
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (uint64_t i = t0; i < 3ull * n_tris; i += stride) {
        const float *v = verts + 3ull * (uint32_t)idx[i];
        for (int k = 0; k < 3; ++k) {
            const uint32_t key = f2key(v[k]);
            lo[k] = min(lo[k], key);
            hi[k] = max(hi[k], key);
        }
    }
    __shared__ uint32_t s_lo[3], s_hi[3];
    if (threadIdx.x < 3) {
        s_lo[threadIdx.x] = 0xFFFFFFFFu;
        s_hi[threadIdx.x] = 0u;
    }
    __syncthreads();
    for (int k = 0; k < 3; ++k) {
        atomicMin(&s_lo[k], lo[k]);
        atomicMax(&s_hi[k], hi[k]);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        atomicMin(&res[RT_REFIT_RES_LO + threadIdx.x], s_lo[threadIdx.x]);
        atomicMax(&res[RT_REFIT_RES_HI + threadIdx.x], s_hi[threadIdx.x]);
    }
    if (bad) atomicOr(&res[RT_REFIT_RES_BAD], bad);
    wave_add(&res[RT_REFIT_RES_NEWLY], newly);
}

/* One lane per record slot of both halves: the record from the slot's original index (r0.w)
   and the new vertices, as k_tri_records forms it; the slot's padded box, as k_prep.
   hit0[s], per tree slot of the closest-hit tree's half: a unit ray could hit the triangle when
   the tree was built — taken from the build's own record by the first update (init). */
__global__ void k_refit_records(const float *__restrict__ verts, const int32_t *__restrict__ idx, uint32_t n_tris,
                                uint32_t n_hit, uint32_t n_recs, float4 *__restrict__ tris, float *__restrict__ tbox,
                                uint8_t *__restrict__ hit0, uint32_t init, uint32_t *__restrict__ res)
{
    const uint32_t s = blockIdx.x * kB + threadIdx.x;
    uint32_t unhit = 0;
    if (s < n_recs) {
        const uint32_t t = __float_as_uint(tris[3ull * s].w);
        if (t >= n_tris) {
            atomicOr(&res[RT_REFIT_RES_BAD], 2u);
        } else {
            if (init && s < n_hit) {
                const float4 r1 = tris[3ull * s + 1], r2 = tris[3ull * s + 2];
                const float o1[3] = {r1.x, r1.y, r1.z}, o2[3] = {r2.x, r2.y, r2.z};
                hit0[s] = never_hit_edges(o1, o2) ? 0 : 1;
            }
            const float *a = verts + 3ull * (uint32_t)idx[3ull * t];
            const float *p1 = verts + 3ull * (uint32_t)idx[3ull * t + 1];
            const float *p2 = verts + 3ull * (uint32_t)idx[3ull * t + 2];
            const float A[3] = {a[0], a[1], a[2]}, P1[3] = {p1[0], p1[1], p1[2]}, P2[3] = {p2[0], p2[1], p2[2]};
            tris[3ull * s] = make_float4(A[0], A[1], A[2], __uint_as_float(t));
            tris[3ull * s + 1] = make_float4(P1[0] - A[0], P1[1] - A[1], P1[2] - A[2], 0.0f);
            tris[3ull * s + 2] = make_float4(P2[0] - A[0], P2[1] - A[1], P2[2] - A[2], 0.0f);
            float lo[3], hi[3], maxabs = 0.0f, ext = 0.0f;
            for (int k = 0; k < 3; ++k) {
                lo[k] = fminf(fminf(A[k], P1[k]), P2[k]);
                hi[k] = fmaxf(fmaxf(A[k], P1[k]), P2[k]);
                maxabs = fmaxf(maxabs, fmaxf(fmaxf(fabsf(A[k]), fabsf(P1[k])), fabsf(P2[k])));
            }
            for (int k = 0; k < 3; ++k) ext = fmaxf(ext, hi[k] - lo[k]);
            const float pad = ext * (1.0f / 512.0f) + 1e-6f * (1.0f + maxabs);
            float *o = tbox + 6ull * s;
            for (int k = 0; k < 3; ++k) {
                o[k] = lo[k] - pad;
                o[3 + k] = hi[k] + pad;
            }
            /* a triangle of the tree that no unit ray can hit any more stays (conservative);
               counted once, in the closest-hit tree's half */
            if (s < n_hit && hit0[s]) unhit = never_hit(A, P1, P2) ? 1u : 0u;
        }
    }
    wave_add(&res[RT_REFIT_RES_UNHIT], unhit);
}

struct NBox { /* k_nbox's (rt_build_gpu.hip) */
    double lo[3], hi[3], err;
};

struct RefitTrees {
    float *full_a;  /* the closest-hit tree's nodes (d_nodes4), n_a of them */
    float *full_s;  /* the shadow tree's full-precision nodes (workspace), node n_a + i at 32 i */
    uint32_t *q4;   /* compressed nodes of both trees (a scratch array for a tree without them) */
    NBox *nb;       /* per node of both trees */
    const float *tris, *tbox;
    uint32_t n_a, n_recs;
    uint32_t det_cull;
    uint32_t *res;
};

__device__ __forceinline__ float *full_node(const RefitTrees &T, uint32_t i)
{
    return i < T.n_a ? T.full_a + 32ull * i : T.full_s + 32ull * (i - T.n_a);
}

__device__ void refit_node(const RefitTrees &T, uint32_t i, uint32_t n_nodes)
{
    float *f = full_node(T, i);
    uint32_t *q = T.q4 + (uint64_t)RT_QNODE_DWORDS * i;
    int32_t code[4];
    for (int k = 0; k < 4; ++k) /* the shadow tree's links live in its compressed nodes alone */
        code[k] = i < T.n_a ? __float_as_int(f[24 + k]) : (int32_t)q[12 + k];
    NBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = __builtin_huge_val();
        b.hi[a] = -__builtin_huge_val();
    }
    b.err = 0.0;
    bool bad = false;
    for (int k = 0; k < 4; ++k) {
        const int32_t c = code[k];
        float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
        if (c != RT_EMPTY_CHILD && c >= 0) {
            if ((uint32_t)c >= n_nodes || (uint32_t)c <= i) {
                bad = true;
            } else {
                const float *cf = full_node(T, (uint32_t)c);
                const uint32_t *cq = T.q4 + (uint64_t)RT_QNODE_DWORDS * (uint32_t)c;
                for (int a = 0; a < 3; ++a) {
                    lo[a] = INFINITY;
                    hi[a] = -INFINITY;
                }
                for (int kk = 0; kk < 4; ++kk) {
                    const int32_t cc = (uint32_t)c < T.n_a ? __float_as_int(cf[24 + kk]) : (int32_t)cq[12 + kk];
                    if (cc == RT_EMPTY_CHILD) continue;
                    for (int a = 0; a < 3; ++a) {
                        lo[a] = fminf(lo[a], cf[8 * a + kk]);
                        hi[a] = fmaxf(hi[a], cf[8 * a + 4 + kk]);
                    }
                }
                const NBox &cb = T.nb[c];
                for (int a = 0; a < 3; ++a) {
                    b.lo[a] = fmin(b.lo[a], cb.lo[a]);
                    b.hi[a] = fmax(b.hi[a], cb.hi[a]);
                }
                b.err = fmax(b.err, cb.err);
            }
        } else if (c != RT_EMPTY_CHILD) {
            const uint32_t enc = (uint32_t)(~c), first = enc >> 3, cnt = (enc & 7u) + 1u;
            if (first + cnt > T.n_recs) {
                bad = true;
            } else {
                for (int a = 0; a < 3; ++a) {
                    lo[a] = INFINITY;
                    hi[a] = -INFINITY;
                }
                for (uint32_t j = 0; j < cnt; ++j) {
                    const float *tb = T.tbox + 6ull * (first + j);
                    for (int a = 0; a < 3; ++a) {
                        lo[a] = fminf(lo[a], tb[a]);
                        hi[a] = fmaxf(hi[a], tb[3 + a]);
                    }
                    const float *o = T.tris + 12ull * (first + j);
                    const double e1[3] = {o[4], o[5], o[6]}, e2[3] = {o[8], o[9], o[10]};
                    const double n[3] = {e2[1] * e1[2] - e2[2] * e1[1], e2[2] * e1[0] - e2[0] * e1[2],
                                         e2[0] * e1[1] - e2[1] * e1[0]};
                    for (int a = 0; a < 3; ++a) {
                        b.lo[a] = fmin(b.lo[a], n[a]);
                        b.hi[a] = fmax(b.hi[a], n[a]);
                    }
                    b.err = fmax(b.err,
                                 (fabs(e1[0]) + fabs(e1[1]) + fabs(e1[2])) * (fabs(e2[0]) + fabs(e2[1]) + fabs(e2[2])));
                }
            }
        }
        for (int a = 0; a < 3; ++a) {
            f[8 * a + k] = lo[a];
            f[8 * a + 4 + k] = hi[a];
        }
        if (i >= T.n_a) {
            f[24 + k] = __int_as_float(c);
            f[28 + k] = 0.0f;
        }
    }
    T.nb[i] = b;
    if (bad) {
        atomicOr(&T.res[RT_REFIT_RES_BAD], 4u);
        return;
    }
    if (!rt_quantize_node4(f, q)) {
        atomicAdd(&T.res[RT_REFIT_RES_QFAIL], 1u);
        return;
    }
    if (T.det_cull) rt_qnode_set_nbox(q, b.lo, b.hi, b.err);
}

/* n_steps levels, deepest first; a step is the nodes of one depth of both trees.  A launch of
   several steps is one block (every step fits it) with a barrier between the levels; a launch
   of one step is a grid over its nodes. */
__global__ void k_refit_levels(RefitTrees T, const RtRefitStep *__restrict__ steps, uint32_t n_steps, uint32_t n_nodes)
{
    for (uint32_t s = 0; s < n_steps; ++s) {
        const RtRefitStep st = steps[s];
        const uint32_t j = blockIdx.x * kB + threadIdx.x;
        if (j < st.a_count) refit_node(T, st.a_first + j, n_nodes);
        else if (j - st.a_count < st.s_count) refit_node(T, st.s_first + (j - st.a_count), n_nodes);
        if (n_steps > 1) __syncthreads();
    }
}

/* Half-areas of the used child boxes of the closest-hit tree, binary64: each block's nodes
   (a fixed share) summed through LDS in a fixed order into part[block]; the host adds the
   partials in index order.  No float atomics: the same tree gives the same bits. */
__global__ void k_refit_area(const float *__restrict__ nodes4, uint32_t n_nodes, double *__restrict__ part)
{
    double sum = 0.0;
    for (uint32_t i = blockIdx.x * kB + threadIdx.x; i < n_nodes; i += gridDim.x * kB) {
        const float *f = nodes4 + 32ull * i;
        for (int k = 0; k < 4; ++k) {
            if (__float_as_int(f[24 + k]) == RT_EMPTY_CHILD) continue;
            const double dx = (double)f[4 + k] - (double)f[k], dy = (double)f[12 + k] - (double)f[8 + k],
                         dz = (double)f[20 + k] - (double)f[16 + k];
            sum += dx * dy + dy * dz + dz * dx;
        }
    }
    __shared__ double s_sum[kB];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int w = kB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = s_sum[0];
}

/* The cone split after a refit: the records of subtree B (slots [first, first + count) of the
   shadow tree's half, as k_refit_records just wrote them) against the lights the split was
   made for.  One parked triangle that a shadow query could now accept and the split no longer
   holds: res[RT_REFIT_RES_CONE] counts them. */
__global__ void k_refit_cone(const float *__restrict__ tris, uint32_t first, uint32_t count,
                             const float *__restrict__ lights, uint32_t n_lights, uint32_t *__restrict__ res)
{
    const uint32_t j = blockIdx.x * kB + threadIdx.x;
    uint32_t can = 0;
    if (j < count) {
        const float *o = tris + 12ull * (first + j);
        const float a[3] = {o[0], o[1], o[2]}, e1[3] = {o[4], o[5], o[6]}, e2[3] = {o[8], o[9], o[10]};
        can = never_occludes_edges(a, e1, e2, lights, n_lights) ? 0u : 1u;
    }
    wave_add(&res[RT_REFIT_RES_CONE], can);
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kB - 1) / kB); }

} // namespace

int rt_launch_refit_cone(const float *tris, uint32_t first, uint32_t count, const float *lights, uint32_t n_lights,
                         uint32_t *res, void *stream)
{
    if (!count) return 0;
    hipLaunchKernelGGL(k_refit_cone, dim3(blocks_for(count)), dim3(kB), 0, (hipStream_t)stream, tris, first, count,
                       lights, n_lights, res);
    return (int)hipGetLastError();
}

int rt_launch_refit_check(const float *verts, uint32_t n_verts, const int32_t *idx, uint32_t n_tris, const float *tris,
                          uint32_t n_hit, uint32_t *res, void *stream)
{
    const uint64_t work = 3ull * (n_verts > n_tris ? n_verts : n_tris);
    unsigned grid = blocks_for(work);
    if (grid > 2048u) grid = 2048u;
    hipLaunchKernelGGL(k_refit_check, dim3(grid), dim3(kB), 0, (hipStream_t)stream, verts, n_verts, idx, n_tris, tris,
                       n_hit, res);
    return (int)hipGetLastError();
}

int rt_launch_refit_records(const float *verts, const int32_t *idx, uint32_t n_tris, uint32_t n_hit, uint32_t n_recs,
                            float *tris, float *tbox, uint8_t *hit0, bool init, uint32_t *res, void *stream)
{
    hipLaunchKernelGGL(k_refit_records, dim3(blocks_for(n_recs)), dim3(kB), 0, (hipStream_t)stream, verts, idx, n_tris,
                       n_hit, n_recs, reinterpret_cast<float4 *>(tris), tbox, hit0, init ? 1u : 0u, res);
    return (int)hipGetLastError();
}

int rt_launch_refit_levels(const RtRefitLaunch &a, const RtRefitStep *steps_dev, const RtRefitStep *steps_host,
                           uint32_t n_steps, void *stream)
{
    RefitTrees T;
    T.full_a = a.nodes4;
    T.full_s = a.nodes4_shadow;
    T.q4 = a.nodes4q;
    T.nb = reinterpret_cast<NBox *>(a.nbox);
    T.tris = a.tris;
    T.tbox = a.tbox;
    T.n_a = a.n_nodes4;
    T.n_recs = a.n_recs;
    T.det_cull = a.det_cull ? 1u : 0u;
    T.res = a.res;
    const uint32_t n_nodes = a.n_nodes4 + a.n_nodes4_shadow;
    for (uint32_t s = 0; s < n_steps;) {
        uint32_t e = s + 1;
        unsigned grid = blocks_for((uint64_t)steps_host[s].a_count + steps_host[s].s_count);
        if (grid <= 1) { /* a run of levels that each fit one block: one launch */
            while (e < n_steps && (uint64_t)steps_host[e].a_count + steps_host[e].s_count <= (uint64_t)kB) ++e;
            grid = 1;
        }
        hipLaunchKernelGGL(k_refit_levels, dim3(grid), dim3(kB), 0, (hipStream_t)stream, T, steps_dev + s, e - s,
                           n_nodes);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return (int)err;
        s = e;
    }
    return 0;
}

int rt_launch_refit_area(const float *nodes4, uint32_t n_nodes4, double *part, void *stream)
{
    hipLaunchKernelGGL(k_refit_area, dim3(RT_REFIT_AREA_BLOCKS), dim3(kB), 0, (hipStream_t)stream, nodes4, n_nodes4,
                       part);
    return (int)hipGetLastError();
}

size_t rt_refit_nbox_bytes(void) { return sizeof(NBox); }
