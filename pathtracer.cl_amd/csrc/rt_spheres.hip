/*
 * rt_spheres.hip — the sphere kernels and the small per-ray / per-row kernels of the MI355X path
 * tracer (the triangle megakernel is rt_tris.hip).
 *
 *   k_spheres<SS>          raytrace / raytrace_ss (clrt/ocl/raytracer.cl:46-104, :120-166), one
 *                          lane per pixel; trace_path (rtcommon.h:267-365) is its path loop
 *   k_trace_rays<TRAV, COUNT>   closest / any-hit queries (rtcommon.h:39-68) of a batch of rays:
 *                          the hit-index parity tests' entry to rt_traverse.h
 *   k_seed_rows            seed-row halo pack / unpack (multi-GPU progressive sphere frames)
 *   rt_launch_spheres, rt_launch_trace_rays, rt_launch_seed_rows
 */
#include <hip/hip_runtime.h>

#include "rt_device.h"
#include "rt_internal.h"
#include "rt_quant.h"
#include "rt_traverse.h"
#include "rt_kernel_util.h"

#pragma clang fp contract(off)

namespace {

/* ======================================================================== */
/* Sphere kernel: raytrace (SS = false) / raytrace_ss (SS = true)            */
/* (raytracer.cl:46-166, trace_path rtcommon.h:267-365).                     */

__device__ V3 trace_path(PathRay &r, const rt_sphere *__restrict__ sph, uint32_t n, uint32_t max_depth, Seed &seed,
                         unsigned long long &n_closest, unsigned long long &n_shadow,
                         unsigned long long &n_skipped)
{
    const float bw = (float)RT_BOX_WIDTH, bh = (float)RT_BOX_HEIGHT;
    V3 color = v3(0.0f, 0.0f, 0.0f);
    for (uint32_t depth = 0; depth <= max_depth; ++depth) {
        ++n_closest;
        /* scene_intersection, rtcommon.h:107-121 */
        int hit = -1;
        for (uint32_t i = 0; i < n; ++i) {
            const float dd = intersect_sphere(r.o, r.d, r.tmin, v3f(sph[i].center), sph[i].radius);
            if (dd > r.tmin && dd < r.tmax) {
                hit = (int)i;
                r.tmax = dd;
            }
        }
        V3 hp, hn;
        float kd = 0.0f;
        V3 diff = v3(0.0f, 0.0f, 0.0f);
        if (hit >= 0) {
            const rt_sphere &s = sph[hit];
            hp = v3(r.o.x + r.d.x * r.tmax, r.o.y + r.d.y * r.tmax, r.o.z + r.d.z * r.tmax);
            const float inv_r = 1.0f / s.radius; /* sphereNormal, geometryFuncs.h:58-69 */
            hn = v3((hp.x - s.center.x) * inv_r, (hp.y - s.center.y) * inv_r, (hp.z - s.center.z) * inv_r);
            if (r.ext.x > 0.0f) r.prop.x *= rt_expf(rt_logf(r.ext.x) * r.tmax);
            if (r.ext.y > 0.0f) r.prop.y *= rt_expf(rt_logf(r.ext.y) * r.tmax);
            if (r.ext.z > 0.0f) r.prop.z *= rt_expf(rt_logf(r.ext.z) * r.tmax);
            if (!r.diffuse && s.mat.emission_power != 0) {
                color.x += r.prop.x * s.mat.emission.x;
                color.y += r.prop.y * s.mat.emission.y;
                color.z += r.prop.z * s.mat.emission.z;
            }
            kd = s.mat.kd;
            diff = v3f(s.mat.diffuse);
        } else {
            const float hd = intersect_box(r.o, r.d, r.tmin, bw, bh, bw);
            if (!(hd > r.tmin && hd < r.tmax)) break;
            r.tmax = hd;
            hp = v3(r.o.x + r.d.x * r.tmax, r.o.y + r.d.y * r.tmax, r.o.z + r.d.z * r.tmax);
            hn = box_normal(hp, bw, bh, bw);
        }
        /* sample_direct_illumination, rtcommon.h:148-174 (box, or kd > 0) */
        V3 direct = v3(0.0f, 0.0f, 0.0f);
        if (hit < 0 || kd > 0.0f) {
            const V3 so = v3(hp.x + hn.x * RT_SMALL_F, hp.y + hn.y * RT_SMALL_F, hp.z + hn.z * RT_SMALL_F);
            const float inv_samples = 1.0f / (float)RT_LIGHT_SAMPLES;
            for (uint32_t k = 0; k < n; ++k) {
                if (sph[k].mat.emission_power != 0) {
                    const V3 lc = v3f(sph[k].center);
                    const float lr = sph[k].radius;
                    for (int i = 0; i < (int)RT_LIGHT_SAMPLES; ++i) {
                        const float r1 = frand(seed);
                        const float r2 = strat_rand(seed, i, (int)RT_LIGHT_SAMPLES);
                        float stmax;
                        const V3 sd = sphere_light_dir(so, lc, lr, r1, r2, stmax);
                        ++n_shadow;
                        /* the light term needs cos(wi) > 0 AND visibility (rtcommon.h:160-167);
                           the const shadow ray is tested only when cos(wi) > 0 — same result */
                        const float cw = sd.x * hn.x + sd.y * hn.y + sd.z * hn.z;
                        bool vis = cw > 0; /* visibility_test, rtcommon.h:128-138 */
                        if (!vis) ++n_skipped;
                        for (uint32_t j = 0; vis && j < n; ++j) {
                            const float dd = intersect_sphere(so, sd, RT_SMALL_F, v3f(sph[j].center), sph[j].radius);
                            if (dd > RT_SMALL_F && dd < stmax) vis = false;
                        }
                        if (vis) {
                            {
                                direct.x += sph[k].mat.emission.x * cw * inv_samples;
                                direct.y += sph[k].mat.emission.y * cw * inv_samples;
                                direct.z += sph[k].mat.emission.z * cw * inv_samples;
                            }
                        }
                    }
                }
            }
        }
        if (hit >= 0) {
            if (kd > 0.0f) {
                const float scale = kd * RT_M_1_PI_F;
                color.x += r.prop.x * direct.x * diff.x * scale;
                color.y += r.prop.y * direct.y * diff.y * scale;
                color.z += r.prop.z * direct.z * diff.z * scale;
            }
            if (depth == max_depth) break;
            if (!sample_material(r, hp, hn, sph[hit].mat, seed)) break;
        } else {
            const float scale = RT_M_1_PI_F;
            r.prop.x *= 0.7f;
            r.prop.y *= 0.7f;
            r.prop.z *= 0.7f;
            color.x += r.prop.x * direct.x * scale;
            color.y += r.prop.y * direct.y * scale;
            color.z += r.prop.z * direct.z * scale;
            r.o = hp;
            r.tmin = RT_SMALL_F;
            r.tmax = kInf;
            const float r1 = frand(seed);
            const float r2 = frand(seed);
            r.d = shading_to_world(cos_sample_hemisphere(r1, r2), hn);
            r.diffuse = 1;
        }
    }
    return color;
}

template <bool SS>
__global__ __launch_bounds__(RT_SPH_TILE * RT_SPH_TILE) void k_spheres(RtSphLaunch a)
{
    /* RT_SPH_TILE x RT_SPH_TILE pixel tile per block; a wave covers 64 consecutive pixels of it */
    const uint32_t x = blockIdx.x * RT_SPH_TILE + (threadIdx.x % RT_SPH_TILE);
    const uint32_t yl = blockIdx.y * RT_SPH_TILE + (threadIdx.x / RT_SPH_TILE);
    unsigned long long n_closest = 0, n_shadow = 0, n_skipped = 0;
    if (x < a.W && yl < a.Hl) {
        const uint32_t y = global_row(a, yl);
        /* get_seed (raytracer.cl:20-24): rows shifted by `progressive`; raytrace_ss unshifted */
        const uint32_t slot = SS ? (y * a.Wpad + x) : (((y + a.progressive) % a.Hpad) * a.Wpad + x);
        Seed seed = load_seed(a, slot);
        const float hw = ((float)a.W) / 2.0f, hh = ((float)a.H) / 2.0f;
        float4 pc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (SS) {
            const float fa = (float)x + frand(seed);
            const float fb = (float)y + frand(seed);
            PathRay r;
            r.o = v3(a.cam.position.x, a.cam.position.y, a.cam.position.z);
            r.d = camera_dir(a.cam, fa - hw, fb - hh);
            r.tmin = RT_SMALL_F;
            r.tmax = kInf;
            r.prop = v3(1.0f, 1.0f, 1.0f);
            r.ext = v3(0.0f, 0.0f, 0.0f);
            r.diffuse = 0;
            const V3 c = trace_path(r, a.spheres, a.n_spheres, a.max_depth, seed, n_closest, n_shadow, n_skipped);
            pc = make_float4(c.x, c.y, c.z, 0.0f);
        } else {
            const uint32_t sr = a.sample_rate;
            for (uint32_t sx = 0; sx < sr; ++sx) {
                for (uint32_t sy = 0; sy < sr; ++sy) {
                    PathRay r;
                    camera_ray(a, seed, x, y, sx, sy, hw, hh, r.o, r.d);
                    r.tmin = RT_SMALL_F;
                    r.tmax = kInf;
                    r.prop = v3(1.0f, 1.0f, 1.0f);
                    r.ext = v3(0.0f, 0.0f, 0.0f);
                    r.diffuse = 0;
                    const V3 c = trace_path(r, a.spheres, a.n_spheres, a.max_depth, seed, n_closest, n_shadow, n_skipped);
                    pc.x += c.x;
                    pc.y += c.y;
                    pc.z += c.z;
                }
            }
            pc = pixel_mean(pc.x, pc.y, pc.z, (float)(sr * sr));
        }
        write_pixel(reinterpret_cast<float4 *>(a.out) + ((size_t)yl * a.W + x), pc, a.progressive > 0,
                    1.0f / (float)a.progressive);
        store_seed(a, slot, seed.x, seed.y);
    }
    unsigned long long cnt[RT_N_COUNTERS] = {};
    cnt[0] = n_closest;
    cnt[1] = n_shadow;
    cnt[RT_CNT_SKIPPED] = n_skipped;
    flush_counters(a.counters, cnt, false);
}

/* ======================================================================== */
/* Batch ray queries (hit-index parity).                                     */
template <int TRAV, bool COUNT>
__global__ __launch_bounds__(RT_BLOCK) void k_trace_rays(const float4 *__restrict__ nodes,
                                                         const float4 *__restrict__ tris, uint32_t n_tris,
                                                         const rt_ray *__restrict__ rays, uint32_t n, int any_hit,
                                                         int32_t *spill, uint32_t spill_cap,
                                                         int32_t *__restrict__ out_idx, float *__restrict__ out_t,
                                                         unsigned long long *__restrict__ counters)
{
    __shared__ int s_stack[RT_STACK_DEPTH * RT_BLOCK];
    const uint32_t i = blockIdx.x * RT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const rt_ray r = rays[i];
    float t = r.tmax;
    TravCounts tc = {0u, 0u, 0u};
    Stack stk;
    stk.init(s_stack, spill, spill_cap);
    const int s = traverse<TRAV, COUNT>(nodes, tris, n_tris, v3f(r.o), v3f(r.d), r.tmin, t, any_hit != 0, stk, tc);
    if (COUNT) { /* counting calls (rt_set_counting): records visited, summed over the rays */
        atomicAdd(&counters[any_hit ? 1 : 0], 1ull);
        atomicAdd(&counters[2], (unsigned long long)tc.nodes);
        atomicAdd(&counters[3], (unsigned long long)tc.tests);
        atomicAdd(&counters[4], (unsigned long long)tc.leaves);
    }
    if (any_hit) {
        out_idx[i] = (s >= 0) ? 1 : 0;
        if (out_t) out_t[i] = r.tmax;
    } else {
        out_idx[i] = (s >= 0) ? __float_as_int(tris[3 * s].w) : -1;
        if (out_t) out_t[i] = t;
    }
}

/* Seed-row halo pack / unpack (multi-GPU progressive sphere frames). */
__global__ __launch_bounds__(RT_BLOCK) void k_seed_rows(uint32_t *__restrict__ seeds, uint32_t wpad, uint32_t hpad,
                                                        const uint32_t *__restrict__ rows, uint32_t n,
                                                        uint32_t *__restrict__ buf, int unpack)
{
    const size_t idx = (size_t)blockIdx.x * RT_BLOCK + threadIdx.x;
    const size_t per_plane = (size_t)n * wpad;
    if (idx >= 2 * per_plane) return;
    const uint32_t p = (uint32_t)(idx / per_plane);
    const uint32_t i = (uint32_t)((idx % per_plane) / wpad);
    const uint32_t x = (uint32_t)(idx % wpad);
    uint32_t *s = seeds + (size_t)p * wpad * hpad + (size_t)rows[i] * wpad + x;
    if (unpack) *s = buf[idx];
    else buf[idx] = *s;
}

} // namespace

int rt_launch_seed_rows(uint32_t *seeds, uint32_t wpad, uint32_t hpad, const uint32_t *rows, uint32_t n,
                        uint32_t *buf, bool unpack, void *stream)
{
    const size_t total = 2ull * n * wpad;
    if (!total) return 0;
    dim3 grid((unsigned)((total + RT_BLOCK - 1) / RT_BLOCK)), block(RT_BLOCK);
    hipLaunchKernelGGL(k_seed_rows, grid, block, 0, (hipStream_t)stream, seeds, wpad, hpad, rows, n, buf,
                       unpack ? 1 : 0);
    return (int)hipGetLastError();
}

int rt_launch_spheres(const RtSphLaunch &a, bool single_sample, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    constexpr uint32_t T = RT_SPH_TILE;
    dim3 grid((a.W + T - 1u) / T, (a.Hl + T - 1u) / T), block(T * T);
    if (single_sample) hipLaunchKernelGGL((k_spheres<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_spheres<false>), grid, block, 0, st, a);
    return (int)hipGetLastError();
}

int rt_launch_trace_rays(const float *nodes, const float *tris, uint32_t n_tris, const rt_ray *rays, uint32_t n,
                         int any_hit, int trav, int32_t *spill, uint32_t spill_cap, int32_t *out_idx, float *out_t,
                         unsigned long long *counters, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((n + RT_BLOCK - 1) / RT_BLOCK), block(RT_BLOCK);
    const float4 *nd = reinterpret_cast<const float4 *>(nodes);
    const float4 *tr = reinterpret_cast<const float4 *>(tris);
#define RT_LAUNCH_TRACE(T)                                                                                             \
    do {                                                                                                               \
        if (counters)                                                                                                  \
            hipLaunchKernelGGL((k_trace_rays<T, true>), grid, block, 0, st, nd, tr, n_tris, rays, n, any_hit, spill,   \
                               spill_cap, out_idx, out_t, counters);                                                   \
        else                                                                                                           \
            hipLaunchKernelGGL((k_trace_rays<T, false>), grid, block, 0, st, nd, tr, n_tris, rays, n, any_hit, spill,  \
                               spill_cap, out_idx, out_t, counters);                                                   \
    } while (0)
    if (trav == RT_TRAV_LINEAR) RT_LAUNCH_TRACE(RT_TRAV_LINEAR);
    else if (trav == RT_TRAV_BVH4Q) RT_LAUNCH_TRACE(RT_TRAV_BVH4Q);
    else RT_LAUNCH_TRACE(RT_TRAV_BVH4);
#undef RT_LAUNCH_TRACE
    return (int)hipGetLastError();
}
