/*
 * rt_features.hip — first-hit feature buffers (gfx950).
 *
 *   k_features<TRAV>   per pixel the first hit of its pixel-centre camera ray: position, depth,
 *                      normal, surface id (the first segment of trace_path_tri, rtcommon.h:380-433)
 *   k_features_sph     the same for the sphere kernels' scene (scene_intersection, rtcommon.h:107-121)
 *
 * Nothing in the reference corresponds to these kernels; their arithmetic is pinned in
 * DESIGN.md §4.9 under the model of include/rt_math.h (no contraction, IEEE division and
 * square root), so that a float32 restatement reproduces every bit.
 * Neither touches a render's state: no seeds, no counters, no queue cursors.
 */
#include <hip/hip_runtime.h>

#include "pathtracer_rt.h"
#include "rt_device.h"
#include "rt_internal.h"
#include "rt_traverse.h"

#pragma clang fp contract(off)

namespace {

/* raytracer.cl:221-224 with the stratified draw replaced by 0.5: the camera ray through the centre
   of pixel (x, y); normalize over the float4 lanes incl. w as the render kernels' camera_dir. */
__device__ __forceinline__ V3 centre_dir(const rt_camera &cam, uint32_t x, uint32_t y, uint32_t W, uint32_t H)
{
    const float a = ((float)x + 0.5f) - ((float)W) / 2.0f;
    const float b = ((float)y + 0.5f) - ((float)H) / 2.0f;
    const float vx = (cam.view.x + cam.right.x * a) + cam.up.x * b;
    const float vy = (cam.view.y + cam.right.y * a) + cam.up.y * b;
    const float vz = (cam.view.z + cam.right.z * a) + cam.up.z * b;
    const float vw = (cam.view.w + cam.right.w * a) + cam.up.w * b;
    const float len = rt_sqrtf(((vx * vx + vy * vy) + vz * vz) + vw * vw);
    return v3(vx / len, vy / len, vz / len);
}

__device__ __forceinline__ void put_feature(const RtFeatLaunch &a, uint32_t p, V3 P, float t, V3 N, int id)
{
    float4 *f = reinterpret_cast<float4 *>(a.feat);
    f[p] = make_float4(P.x, P.y, P.z, t);
    f[(size_t)a.W * a.H + p] = make_float4(N.x, N.y, N.z, __int_as_float(id));
}

/* the enclosing box behind everything else (rtcommon.h:423-433), or no surface at all */
__device__ __forceinline__ void box_or_none(const RtFeatLaunch &a, uint32_t p, V3 o, V3 d)
{
    const float bw = (float)RT_BOX_WIDTH, bh = (float)RT_BOX_HEIGHT;
    const float hd = intersect_box(o, d, RT_SMALL_F, bw, bh, bw);
    if (hd > RT_SMALL_F && hd < kInf) {
        const V3 hp = v3(o.x + d.x * hd, o.y + d.y * hd, o.z + d.z * hd);
        put_feature(a, p, hp, hd, box_normal(hp, bw, bh, bw), RT_FEAT_BOX);
    } else {
        put_feature(a, p, v3(0.0f, 0.0f, 0.0f), kInf, v3(0.0f, 0.0f, 0.0f), RT_FEAT_NONE);
    }
}

/* One lane per pixel, row-major; the closest-hit query is k_trace_rays's (per-lane traverse<>, LDS
   stack, the context's spill area indexed by block). */
template <int TRAV>
__global__ __launch_bounds__(RT_BLOCK) void k_features(RtFeatLaunch a)
{
    __shared__ int s_stack[RT_STACK_DEPTH * RT_BLOCK];
    const uint32_t p = blockIdx.x * RT_BLOCK + threadIdx.x;
    if (p >= a.W * a.H) return;
    const uint32_t x = p % a.W, y = p / a.W;
    const V3 o = v3(a.cam.position.x, a.cam.position.y, a.cam.position.z);
    const V3 d = centre_dir(a.cam, x, y, a.W, a.H);
    const float4 *tris = reinterpret_cast<const float4 *>(a.tris);
    float t = kInf;
    TravCounts tc = {0u, 0u, 0u};
    Stack stk;
    stk.init(s_stack, a.spill, a.spill_cap);
    const int s = traverse<TRAV, false>(reinterpret_cast<const float4 *>(a.nodes), tris, a.n_tris, o, d, RT_SMALL_F,
                                        t, false, stk, tc);
    if (s >= 0) {
        const float4 r0 = tris[3 * s], e1 = tris[3 * s + 1], e2 = tris[3 * s + 2];
        /* the reference's unnormalised normal (rtcommon.h:389), normalised; never flipped */
        const V3 n = cross3(v3(e2.x, e2.y, e2.z), v3(e1.x, e1.y, e1.z));
        const float len = rt_sqrtf(dot3(n, n));
        put_feature(a, p, v3(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t), t, v3(n.x / len, n.y / len, n.z / len),
                    __float_as_int(r0.w));
    } else {
        box_or_none(a, p, o, d);
    }
}

__global__ __launch_bounds__(RT_BLOCK) void k_features_sph(RtFeatLaunch a)
{
    const uint32_t p = blockIdx.x * RT_BLOCK + threadIdx.x;
    if (p >= a.W * a.H) return;
    const uint32_t x = p % a.W, y = p / a.W;
    const V3 o = v3(a.cam.position.x, a.cam.position.y, a.cam.position.z);
    const V3 d = centre_dir(a.cam, x, y, a.W, a.H);
    /* scene_intersection, rtcommon.h:107-121: strict interval, the lowest index on ties */
    int hit = -1;
    float tmax = kInf;
    for (uint32_t i = 0; i < a.n_spheres; ++i) {
        const float dd = intersect_sphere(o, d, RT_SMALL_F, v3f(a.spheres[i].center), a.spheres[i].radius);
        if (dd > RT_SMALL_F && dd < tmax) {
            hit = (int)i;
            tmax = dd;
        }
    }
    if (hit >= 0) {
        const rt_sphere &s = a.spheres[hit];
        const V3 hp = v3(o.x + d.x * tmax, o.y + d.y * tmax, o.z + d.z * tmax);
        const float inv_r = 1.0f / s.radius; /* sphereNormal, geometryFuncs.h:58-69, as k_spheres */
        put_feature(a, p, hp, tmax,
                    v3((hp.x - s.center.x) * inv_r, (hp.y - s.center.y) * inv_r, (hp.z - s.center.z) * inv_r),
                    RT_FEAT_SPHERE0 - hit);
    } else {
        box_or_none(a, p, o, d);
    }
}

} // namespace

int rt_launch_features(const RtFeatLaunch &a, int trav, void *stream)
{
    const uint64_t npx = (uint64_t)a.W * a.H;
    const dim3 grid((uint32_t)((npx + RT_BLOCK - 1) / RT_BLOCK)), block(RT_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    if (a.spheres) hipLaunchKernelGGL(k_features_sph, grid, block, 0, st, a);
    else if (trav == RT_TRAV_LINEAR) hipLaunchKernelGGL((k_features<RT_TRAV_LINEAR>), grid, block, 0, st, a);
    else if (trav == RT_TRAV_BVH4) hipLaunchKernelGGL((k_features<RT_TRAV_BVH4>), grid, block, 0, st, a);
    else if (trav == RT_TRAV_BVH4Q) hipLaunchKernelGGL((k_features<RT_TRAV_BVH4Q>), grid, block, 0, st, a);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}
