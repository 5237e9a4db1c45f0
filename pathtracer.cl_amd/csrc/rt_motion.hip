/*
 * rt_motion.hip — first-hit features of a moving mesh or of moved spheres, rewritten into an earlier
 * pose (gfx950).
 *
 *   k_warp_features   per pixel of the current view's feature buffer: a mesh pixel's hit point as
 *                     barycentrics of its triangle in the current pose, then position and normal of
 *                     that material point in an earlier pose of the same mesh (same indices).
 *                     rt_reproject, given the result as its cur_feat, carries the history that is
 *                     attached to the material, not to the place.
 *   k_warp_features_sph   the sphere twin: a sphere pixel's hit point, which the features hold as the
 *                     unit normal N = (P - C) / r, put back on the sphere of the same index in an
 *                     earlier list of spheres: P' = C' + N r'.
 *
 * Nothing in the reference corresponds to these kernels; their arithmetic is pinned in DESIGN.md §4.13
 * and §4.16 under the model of include/rt_math.h (no contraction, IEEE division and square root), so
 * that a float32 restatement reproduces every bit.  They touch no render state, and write nothing but
 * out_feat (which may be cur_feat: a lane reads its own pixel before it writes it).
 */
#include <hip/hip_runtime.h>

#include "pathtracer_rt.h"
#include "rt_device.h"
#include "rt_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr float kInf = __builtin_huge_valf();

struct WarpArgs {
    const float4 *cur;
    float4 *out;
    const int32_t *idx; /* 3 per triangle, the caller's numbering */
    const float *pose;  /* the current pose, 3 floats per vertex */
    const float *prev;  /* the earlier pose */
    uint32_t npx, n_tris, n_verts;
};

RTD V3 vert(const float *v, uint32_t i) { return v3(v[3ull * i], v[3ull * i + 1], v[3ull * i + 2]); }
RTD V3 sub3(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
RTD bool finite3(V3 a) { return rt_fabsf(a.x) < kInf && rt_fabsf(a.y) < kInf && rt_fabsf(a.z) < kInf; } /* false for a NaN */

/* One lane per pixel, row-major as k_features.  No address is formed from the pixel's id or from
   an index before it has been compared with n_tris / n_verts. */
__global__ __launch_bounds__(RT_BLOCK) void k_warp_features(WarpArgs a)
{
    const uint32_t p = blockIdx.x * RT_BLOCK + threadIdx.x;
    if (p >= a.npx) return;
    float4 o0 = a.cur[p], o1 = a.cur[(size_t)a.npx + p];
    const int id = __float_as_int(o1.w);
    if (id >= 0) { /* a mesh pixel; box, spheres and none are copied bit for bit */
        bool ok = false;
        if ((uint32_t)id < a.n_tris) {
            const int32_t *ix = a.idx + 3ull * (uint32_t)id;
            const uint32_t i0 = (uint32_t)ix[0], i1 = (uint32_t)ix[1], i2 = (uint32_t)ix[2]; /* negative: above n_verts */
            if (i0 < a.n_verts && i1 < a.n_verts && i2 < a.n_verts) {
                /* the hit point's barycentrics in the current pose, through the triangle's normal */
                const V3 va = vert(a.pose, i0);
                const V3 e1 = sub3(vert(a.pose, i1), va), e2 = sub3(vert(a.pose, i2), va);
                const V3 w = sub3(v3(o0.x, o0.y, o0.z), va);
                const V3 n = cross3(e1, e2);
                const float nn = dot3(n, n);
                const float u = dot3(cross3(w, e2), n) / nn, v = dot3(cross3(e1, w), n) / nn;
                /* the same point and k_features' normal in the earlier pose */
                const V3 pa = vert(a.prev, i0);
                const V3 f1 = sub3(vert(a.prev, i1), pa), f2 = sub3(vert(a.prev, i2), pa);
                const V3 P = v3((pa.x + f1.x * u) + f2.x * v, (pa.y + f1.y * u) + f2.y * v, (pa.z + f1.z * u) + f2.z * v);
                const V3 m = cross3(f2, f1);
                const float len = rt_sqrtf(dot3(m, m));
                const V3 N = v3(m.x / len, m.y / len, m.z / len);
                if (nn != 0.0f && len > 0.0f && finite3(P) && finite3(N)) {
                    ok = true;
                    o0 = make_float4(P.x, P.y, P.z, o0.w);
                    o1 = make_float4(N.x, N.y, N.z, o1.w);
                }
            }
        }
        if (!ok) { /* no surface: rt_reproject gives it no history */
            o0 = make_float4(0.0f, 0.0f, 0.0f, kInf);
            o1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(RT_FEAT_NONE));
        }
    }
    a.out[p] = o0;
    a.out[(size_t)a.npx + p] = o1;
}

struct SphWarpArgs {
    const float4 *cur;
    float4 *out;
    const rt_sphere *sph;  /* the current spheres */
    const rt_sphere *prev; /* the earlier ones */
    uint32_t npx, n_cur, n_prev;
};

/* One lane per pixel, row-major as k_features_sph.  No address is formed from the pixel's id before
   the sphere index it names has been compared with both counts. */
__global__ __launch_bounds__(RT_BLOCK) void k_warp_features_sph(SphWarpArgs a)
{
    const uint32_t p = blockIdx.x * RT_BLOCK + threadIdx.x;
    if (p >= a.npx) return;
    float4 o0 = a.cur[p], o1 = a.cur[(size_t)a.npx + p];
    const int id = __float_as_int(o1.w);
    if (id <= RT_FEAT_SPHERE0) { /* a sphere pixel; mesh, box, none and the unused ids are copied bit for bit */
        const uint32_t s = (uint32_t)RT_FEAT_SPHERE0 - (uint32_t)id; /* modulo 2^32: INT32_MIN gives 2^31 - 16 */
        bool ok = false;
        if (s < a.n_cur && s < a.n_prev) {
            const rt_sphere &c = a.sph[s], &q = a.prev[s];
            const float r = q.radius;
            if (__float_as_uint(c.center.x) == __float_as_uint(q.center.x) && __float_as_uint(c.center.y) == __float_as_uint(q.center.y) &&
                __float_as_uint(c.center.z) == __float_as_uint(q.center.z) && __float_as_uint(c.radius) == __float_as_uint(r)) {
                ok = true; /* it stands where it stood: the input's bits */
            } else {
                const V3 P = v3(q.center.x + o1.x * r, q.center.y + o1.y * r, q.center.z + o1.z * r);
                if (r > 0.0f && r < kInf && finite3(P)) { /* (r > 0 is false for a NaN) */
                    ok = true;
                    o0 = make_float4(P.x, P.y, P.z, o0.w);
                }
            }
        }
        if (!ok) { /* no surface: rt_reproject gives it no history */
            o0 = make_float4(0.0f, 0.0f, 0.0f, kInf);
            o1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(RT_FEAT_NONE));
        }
    }
    a.out[p] = o0;
    a.out[(size_t)a.npx + p] = o1;
}

} // namespace

int rt_launch_warp_features(const float *cur_feat, const int32_t *idx, const float *pose, const float *prev_verts,
                            uint32_t n_tris, uint32_t n_verts, float *out_feat, uint32_t W, uint32_t H, void *stream)
{
    WarpArgs a;
    a.cur = reinterpret_cast<const float4 *>(cur_feat);
    a.out = reinterpret_cast<float4 *>(out_feat);
    a.idx = idx;
    a.pose = pose;
    a.prev = prev_verts;
    a.npx = W * H; /* < 2^28 (the host's frame check) */
    a.n_tris = n_tris;
    a.n_verts = n_verts;
    hipLaunchKernelGGL(k_warp_features, dim3((a.npx + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int rt_launch_warp_features_spheres(const float *cur_feat, const rt_sphere *spheres, uint32_t n_cur, const rt_sphere *prev_spheres,
                                    uint32_t n_prev, float *out_feat, uint32_t W, uint32_t H, void *stream)
{
    SphWarpArgs a;
    a.cur = reinterpret_cast<const float4 *>(cur_feat);
    a.out = reinterpret_cast<float4 *>(out_feat);
    a.sph = spheres;
    a.prev = prev_spheres;
    a.npx = W * H; /* < 2^28 (the host's frame check) */
    a.n_cur = n_cur;
    a.n_prev = n_prev;
    hipLaunchKernelGGL(k_warp_features_sph, dim3((a.npx + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
