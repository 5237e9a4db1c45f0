/*
 * rt_denoise.hip — first-hit feature buffers and the edge-avoiding display filter (gfx950).
 *
 *   k_features<TRAV>   per pixel the first hit of its pixel-centre camera ray: position, depth,
 *                      normal, surface id (the first segment of trace_path_tri, rtcommon.h:380-433)
 *   k_features_sph     the same for the sphere kernels' scene (scene_intersection, rtcommon.h:107-121)
 *   k_atrous, k_atrous_lds<S>   one pass of the a-trous wavelet filter (Dammertz et al. 2010) guided by
 *                      them: taps gathered from global memory, or (steps 1 and 2) from a tile staged in LDS
 *
 * Nothing in the reference corresponds to these kernels; their arithmetic is pinned in
 * DESIGN.md §4.9 under the model of include/rt_math.h (no contraction, IEEE division and
 * square root, the pinned exponential), so that a float32 restatement reproduces every bit.
 * Neither touches a render's state: no seeds, no counters, no queue cursors.
 */
#include <hip/hip_runtime.h>

#include <cstdlib>

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

/* ---- the filter.  Tap order and arithmetic as DESIGN.md §4.9: dy outer, dx inner, a tap outside the
   frame skipped; how the three float4 streams of a tap (colour, P, N) reach the lane is the kernels'. */
struct AtrousAcc {
    float x, y, z, wsum;
};

/* one tap: w = h exp(-((ec isc + en isn) + ep isp)), acc += c_q w */
__device__ __forceinline__ void atrous_tap(AtrousAcc &acc, float h, float4 cq, float4 pq, float4 nq, float4 cp,
                                           float4 pp, float4 np, float isc, float isn, float isp)
{
    const float dcx = cq.x - cp.x, dcy = cq.y - cp.y, dcz = cq.z - cp.z;
    const float ec = dcx * dcx + dcy * dcy + dcz * dcz;
    const float dnx = nq.x - np.x, dny = nq.y - np.y, dnz = nq.z - np.z;
    const float en = dnx * dnx + dny * dny + dnz * dnz;
    const float pl = (pq.x - pp.x) * np.x + (pq.y - pp.y) * np.y + (pq.z - pp.z) * np.z;
    const float ep = pl * pl;
    const float w = h * rt_expf(-((ec * isc + en * isn) + ep * isp));
    acc.x += cq.x * w;
    acc.y += cq.y * w;
    acc.z += cq.z * w;
    acc.wsum += w;
}

__device__ __forceinline__ float atrous_h(int dx, int dy)
{
    const float k[3] = {0.375f, 0.25f, 0.0625f};
    return k[dx < 0 ? -dx : dx] * k[dy < 0 ? -dy : dy];
}

/* One lane per pixel; a block covers RT_ATROUS_BX x RT_ATROUS_BY pixels, a wave two rows of 32
   (512-B row segments per float4 stream). */
#define RT_ATROUS_BX 32
#define RT_ATROUS_BY 8

/* The gather form (steps 4 and up): the 25 taps straight from global memory — the re-reads of lines
   the neighbours fetch are served by the vector L1 / L2, the frame's three streams fit the Infinity
   Cache; a halo of 2 step pixels around a block's tile would not fit LDS from step 8 on. */
__global__ __launch_bounds__(RT_ATROUS_BX *RT_ATROUS_BY) void k_atrous(const float4 *__restrict__ col,
                                                                        const float4 *__restrict__ feat,
                                                                        float4 *__restrict__ out, uint32_t W, uint32_t H,
                                                                        int step, float isc, float isn, float isp)
{
    const int x = (int)(blockIdx.x * RT_ATROUS_BX + threadIdx.x);
    const int y = (int)(blockIdx.y * RT_ATROUS_BY + threadIdx.y);
    if (x >= (int)W || y >= (int)H) return;
    const float4 *__restrict__ pos = feat;
    const float4 *__restrict__ nrm = feat + (size_t)W * H;
    const size_t p = (size_t)y * W + x;
    const float4 cp = col[p], pp = pos[p], np = nrm[p];
    AtrousAcc acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + step * dy;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= (int)W || qy < 0 || qy >= (int)H) continue;
            const size_t q = (size_t)qy * W + qx;
            atrous_tap(acc, atrous_h(dx, dy), col[q], pos[q], nrm[q], cp, pp, np, isc, isn, isp);
        }
    }
    out[p] = make_float4(acc.x / acc.wsum, acc.y / acc.wsum, acc.z / acc.wsum, cp.w);
}

/* The staged form (steps S = 1 and 2): the block's tile and its halo of 2 S pixels — (32 + 4 S) x
   (8 + 4 S) pixels of the three streams, 20 KB / 30 KB — loaded once into LDS, the taps read from
   there (consecutive lanes read consecutive 16-B cells: conflict-free ds_read_b128).  Cells outside
   the frame are neither written nor read.  Measured 25 % / 22 % faster than the gather form at these
   two steps (profiles/denoise). */
template <int S>
__global__ __launch_bounds__(RT_ATROUS_BX *RT_ATROUS_BY) void k_atrous_lds(const float4 *__restrict__ col,
                                                                            const float4 *__restrict__ feat,
                                                                            float4 *__restrict__ out, uint32_t W,
                                                                            uint32_t H, float isc, float isn, float isp)
{
    constexpr int TW = RT_ATROUS_BX + 4 * S, TH = RT_ATROUS_BY + 4 * S;
    __shared__ float4 s_c[TW * TH], s_p[TW * TH], s_n[TW * TH];
    const float4 *__restrict__ pos = feat;
    const float4 *__restrict__ nrm = feat + (size_t)W * H;
    const int x0 = (int)(blockIdx.x * RT_ATROUS_BX) - 2 * S, y0 = (int)(blockIdx.y * RT_ATROUS_BY) - 2 * S;
    const int tid = (int)(threadIdx.y * RT_ATROUS_BX + threadIdx.x);
    for (int i = tid; i < TW * TH; i += RT_ATROUS_BX * RT_ATROUS_BY) {
        const int gx = x0 + i % TW, gy = y0 + i / TW;
        if (gx >= 0 && gx < (int)W && gy >= 0 && gy < (int)H) {
            const size_t q = (size_t)gy * W + gx;
            s_c[i] = col[q];
            s_p[i] = pos[q];
            s_n[i] = nrm[q];
        }
    }
    __syncthreads();
    const int x = (int)(blockIdx.x * RT_ATROUS_BX + threadIdx.x);
    const int y = (int)(blockIdx.y * RT_ATROUS_BY + threadIdx.y);
    if (x >= (int)W || y >= (int)H) return;
    const int lp = ((int)threadIdx.y + 2 * S) * TW + (int)threadIdx.x + 2 * S;
    const float4 cp = s_c[lp], pp = s_p[lp], np = s_n[lp];
    AtrousAcc acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + S * dy;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + S * dx;
            if (qx < 0 || qx >= (int)W || qy < 0 || qy >= (int)H) continue;
            const int q = lp + S * dy * TW + S * dx;
            atrous_tap(acc, atrous_h(dx, dy), s_c[q], s_p[q], s_n[q], cp, pp, np, isc, isn, isp);
        }
    }
    out[(size_t)y * W + x] = make_float4(acc.x / acc.wsum, acc.y / acc.wsum, acc.z / acc.wsum, cp.w);
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

int rt_launch_atrous(const float *col, const float *feat, float *out, uint32_t W, uint32_t H, uint32_t step, float isc,
                     float isn, float isp, void *stream)
{
    const dim3 grid((W + RT_ATROUS_BX - 1) / RT_ATROUS_BX, (H + RT_ATROUS_BY - 1) / RT_ATROUS_BY);
    const dim3 block(RT_ATROUS_BX, RT_ATROUS_BY);
    /* steps 1 and 2 from LDS, the larger ones gathered (the step size decides: profiles/denoise);
       RTMI_ATROUS_LDS (A/B knob, no result bit depends on it): the largest step staged, 0 = none */
    const char *knob = getenv("RTMI_ATROUS_LDS");
    const uint32_t lds_max = knob ? (uint32_t)atoi(knob) : 2u;
    if (step <= 2 && step <= lds_max) {
        if (step == 1)
            hipLaunchKernelGGL(k_atrous_lds<1>, grid, block, 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(col),
                               reinterpret_cast<const float4 *>(feat), reinterpret_cast<float4 *>(out), W, H, isc, isn, isp);
        else
            hipLaunchKernelGGL(k_atrous_lds<2>, grid, block, 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(col),
                               reinterpret_cast<const float4 *>(feat), reinterpret_cast<float4 *>(out), W, H, isc, isn, isp);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(k_atrous, grid, block, 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(col),
                       reinterpret_cast<const float4 *>(feat), reinterpret_cast<float4 *>(out), W, H, (int)step, isc,
                       isn, isp);
    return (int)hipGetLastError();
}
