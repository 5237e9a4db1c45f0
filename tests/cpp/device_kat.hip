/*
 * device_kat.hip — TEST MODULE (tests/cpp/libdevkat.so; never part of librtmi.so).
 *
 * The device build of the pinned arithmetic model (include/rt_math.h) and of the sampling,
 * shading and intersection helpers (csrc/rt_device.h, rt_traverse.h, rt_kernel_util.h),
 * evaluated function by function: every kernel below calls the very function the render kernels
 * call, one thread per element, and the host compares the results bit for bit with the CPU oracle
 * (tests/test_gpu_device_kat.py).  Compiled with the library's own COMMON and DEVFLAGS
 * (tests/cpp/Makefile reads them from csrc/Makefile), so a changed flag changes this module too.
 *
 * Every entry: host arrays in, one launch of 256-thread blocks with a bounds guard, results out,
 * the HIP status returned (0 = hipSuccess).  Records are the C ABI's (include/rt_types.h).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "rt_device.h"
#include "rt_internal.h"
#include "rt_quant.h"
#include "rt_traverse.h"
#include "rt_kernel_util.h"

#pragma clang fp contract(off)

#define DK_API extern "C" __attribute__((visibility("default")))

namespace {

/* Device copies of one entry's arrays; the first failing HIP call sticks and skips the rest. */
class Dev {
    std::vector<void *> bufs_;
    hipError_t st_ = hipSuccess;

public:
    ~Dev()
    {
        for (void *p : bufs_) (void)hipFree(p);
    }
    bool ok() const { return st_ == hipSuccess; }
    int status() const { return (int)st_; }
    template <class T> T *alloc(size_t n)
    {
        void *p = nullptr;
        if (ok()) st_ = hipMalloc(&p, (n ? n : 1) * sizeof(T));
        if (!ok()) return nullptr;
        bufs_.push_back(p);
        return (T *)p;
    }
    template <class T> T *in(const T *h, size_t n)
    {
        T *d = alloc<T>(n);
        if (ok() && n) st_ = hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    template <class T> void out(T *h, const T *d, size_t n)
    {
        if (ok() && n) st_ = hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
    }
    void launched()
    {
        if (ok()) st_ = hipGetLastError();
        if (ok()) st_ = hipDeviceSynchronize();
    }
};

#define DK_LAUNCH(dev, n, kern, ...)                                                                        \
    do {                                                                                                    \
        if ((dev).ok() && (n)) {                                                                            \
            hipLaunchKernelGGL(kern, dim3((unsigned)(((size_t)(n) + 255u) / 256u)), dim3(256), 0, 0,        \
                               __VA_ARGS__);                                                                \
            (dev).launched();                                                                               \
        }                                                                                                   \
    } while (0)

#define DK_INDEX(n)                                             \
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;         \
    if (i >= (n)) return

__device__ __forceinline__ V3 ld3(const float *p, uint32_t i) { return v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
__device__ __forceinline__ void st3(float *p, uint32_t i, V3 v)
{
    p[3 * i] = v.x;
    p[3 * i + 1] = v.y;
    p[3 * i + 2] = v.z;
}
__device__ __forceinline__ rt_vec3 to_vec3(V3 v)
{
    rt_vec3 r;
    r.x = v.x;
    r.y = v.y;
    r.z = v.z;
    return r;
}
__device__ __forceinline__ PathRay to_path(const rt_ray &r)
{
    PathRay p;
    p.o = v3f(r.o);
    p.d = v3f(r.d);
    p.tmin = r.tmin;
    p.tmax = r.tmax;
    p.prop = v3f(r.propagation);
    p.ext = v3f(r.extinction);
    p.diffuse = r.diffuse_bounce;
    return p;
}
__device__ __forceinline__ rt_ray from_path(const PathRay &p)
{
    rt_ray r;
    r.o = to_vec3(p.o);
    r.d = to_vec3(p.d);
    r.tmin = p.tmin;
    r.tmax = p.tmax;
    r.propagation = to_vec3(p.prop);
    r.extinction = to_vec3(p.ext);
    r.diffuse_bounce = p.diffuse;
    return r;
}

/* ---- math: the codes of oracle/pt_oracle.c or_math_vec ------------------ */
enum {
    DK_SIN = 0, DK_COS, DK_EXP, DK_LOG, DK_POW_Y0, DK_SINCOS_S, DK_SINCOS_C, DK_POW, DK_SQRT, DK_RSQRT, DK_LDEXP,
    DK_DIV, DK_MIN, DK_MAX, DK_N_MATH
};

template <int FN> __global__ void k_math(const float *x, const float *y, float *out, uint32_t n)
{
    DK_INDEX(n);
    float s, c, r;
    if (FN == DK_SIN) r = rt_sinf(x[i]);
    else if (FN == DK_COS) r = rt_cosf(x[i]);
    else if (FN == DK_EXP) r = rt_expf(x[i]);
    else if (FN == DK_LOG) r = rt_logf(x[i]);
    else if (FN == DK_POW_Y0) r = rt_powf(x[i], y[0]);
    else if (FN == DK_SINCOS_S) { rt_sincosf(x[i], &s, &c); r = s; }
    else if (FN == DK_SINCOS_C) { rt_sincosf(x[i], &s, &c); r = c; }
    else if (FN == DK_POW) r = rt_powf(x[i], y[i]);
    else if (FN == DK_SQRT) r = rt_sqrtf(x[i]);
    else if (FN == DK_RSQRT) r = rt_rsqrtf(x[i]);
    else if (FN == DK_LDEXP) r = rt_ldexpf(x[i], ((const int32_t *)y)[i]);
    else if (FN == DK_DIV) r = x[i] / y[i];
    else if (FN == DK_MIN) r = rt_minf(x[i], y[i]);
    else r = rt_maxf(x[i], y[i]);
    out[i] = r;
}

/* ---- rng ------------------------------------------------------------------ */
template <bool STRAT>
__global__ void k_rand(const uint32_t *seeds, uint32_t k, int total, float *vals, uint32_t *seeds_out, uint32_t n)
{
    DK_INDEX(n);
    Seed s;
    s.x = seeds[2 * i];
    s.y = seeds[2 * i + 1];
    for (uint32_t j = 0; j < k; ++j)
        vals[(size_t)i * k + j] = STRAT ? strat_rand(s, (int)(j % (uint32_t)total), total) : frand(s);
    seeds_out[2 * i] = s.x;
    seeds_out[2 * i + 1] = s.y;
}

template <uint32_t A>
__global__ void k_mwc_jump(const uint32_t *x, const uint32_t *k, const uint32_t *mul, uint32_t *out, uint32_t n)
{
    DK_INDEX(n);
    out[i] = mwc_jump<A>(x[i], k[i], mul[i]);
}

/* ---- geometry ------------------------------------------------------------- */
/* mt_test, then the leaf loop's acceptance (rt_traverse.h leaf_accept) of a lone triangle of
   original index 0 against the ray's own interval: the closest-hit and the any-hit form. */
__global__ void k_mt_test(const rt_ray *rays, const rt_triangle *tris, int32_t *hit, float *t_out, int32_t *hit_any,
                          uint32_t n)
{
    DK_INDEX(n);
    const rt_ray r = rays[i];
    const rt_triangle tr = tris[i];
    const V3 o = v3f(r.o), d = v3f(r.d);
    const float4 a = make_float4(tr.v0.x, tr.v0.y, tr.v0.z, __int_as_float(0));
    const float4 b = make_float4(tr.e1.x, tr.e1.y, tr.e1.z, 0.0f);
    const float4 c = make_float4(tr.e2.x, tr.e2.y, tr.e2.z, 0.0f);
    float t = 0.0f;
    const bool ok = mt_test(o, d, a, b, c, t);
    int best = -1, best_orig = -1;
    float best_t = r.tmax;
    bool done = false;
    leaf_accept<false>(0, a, d, ok, t, r.tmin, r.tmax, false, best, best_orig, best_t, done);
    hit[i] = best >= 0;
    t_out[i] = best_t;
    best = -1;
    best_orig = -1;
    float any_t = r.tmax;
    done = false;
    leaf_accept<false>(0, a, d, ok, t, r.tmin, r.tmax, true, best, best_orig, any_t, done);
    hit_any[i] = done;
}

__global__ void k_sphere(const rt_ray *rays, const float *c, const float *radius, float *out, uint32_t n)
{
    DK_INDEX(n);
    const rt_ray r = rays[i];
    out[i] = intersect_sphere(v3f(r.o), v3f(r.d), r.tmin, ld3(c, i), radius[i]);
}

/* intersect_box, then box_normal at o + d t where t is finite (a miss returns 0 or inf: 0 leaves
   the origin itself, inf has no point and writes a zero normal). */
__global__ void k_box(const rt_ray *rays, float xs, float ys, float zs, float *t_out, float *nrm, uint32_t n)
{
    DK_INDEX(n);
    const rt_ray r = rays[i];
    const float t = intersect_box(v3f(r.o), v3f(r.d), r.tmin, xs, ys, zs);
    t_out[i] = t;
    V3 nn = v3(0.0f, 0.0f, 0.0f);
    if (rt_fabsf(t) < rt_inff()) {
        const V3 p = v3(r.o.x + r.d.x * t, r.o.y + r.d.y * t, r.o.z + r.d.z * t);
        nn = box_normal(p, xs, ys, zs);
    }
    st3(nrm, i, nn);
}

__global__ void k_camera_dir(const rt_camera *cams, const int32_t *cam_idx, const float *a, const float *b,
                             float *out, uint32_t n)
{
    DK_INDEX(n);
    st3(out, i, camera_dir(cams[cam_idx[i]], a[i], b[i]));
}

/* ---- frames and sampling --------------------------------------------------- */
template <int FN> __global__ void k_frame(const float *v, const float *nrm, float *out, uint32_t n)
{
    DK_INDEX(n);
    V3 r;
    if (FN == 0) r = perpendicular(ld3(v, i));
    else if (FN == 1) r = shading_to_world(ld3(v, i), ld3(nrm, i));
    else r = world_to_shading(ld3(v, i), ld3(nrm, i));
    st3(out, i, r);
}

__global__ void k_cos_sample_hemisphere(const float *r1, const float *r2, float *out, uint32_t n)
{
    DK_INDEX(n);
    st3(out, i, cos_sample_hemisphere(r1[i], r2[i]));
}

__global__ void k_sample_phong(const float *w, const float *spec_exp, const float *r1, const float *r2, float *out,
                               uint32_t n)
{
    DK_INDEX(n);
    st3(out, i, sample_phong(ld3(w, i), spec_exp[i], r1[i], r2[i]));
}

__global__ void k_sample_refraction(rt_ray *rays, const float *ior, const float *blur_exp, const float *r1,
                                    const float *r2, int32_t *ret, uint32_t n)
{
    DK_INDEX(n);
    PathRay p = to_path(rays[i]);
    ret[i] = sample_refraction(p, ior[i], blur_exp[i], r1[i], r2[i]) ? 1 : 0;
    rays[i] = from_path(p);
}

__global__ void k_sphere_light_dir(const float *o, const float *c, const float *radius, const float *r1,
                                   const float *r2, float *dir, float *tmax, uint32_t n)
{
    DK_INDEX(n);
    float tm = 0.0f;
    st3(dir, i, sphere_light_dir(ld3(o, i), ld3(c, i), radius[i], r1[i], r2[i], tm));
    tmax[i] = tm;
}

__global__ void k_sample_material(rt_ray *rays, const float *hits, const rt_material *mats, const int32_t *mat_idx,
                                  uint32_t *seeds, int32_t *ret, uint32_t n)
{
    DK_INDEX(n);
    PathRay p = to_path(rays[i]);
    Seed s;
    s.x = seeds[2 * i];
    s.y = seeds[2 * i + 1];
    const V3 hp = v3(hits[6 * i], hits[6 * i + 1], hits[6 * i + 2]);
    const V3 nn = v3(hits[6 * i + 3], hits[6 * i + 4], hits[6 * i + 5]);
    ret[i] = sample_material(p, hp, nn, mats[mat_idx[i]], s) ? 1 : 0;
    rays[i] = from_path(p);
    seeds[2 * i] = s.x;
    seeds[2 * i + 1] = s.y;
}

template <int FN> void launch_math(Dev &dev, const float *x, const float *y, float *out, uint32_t n)
{
    DK_LAUNCH(dev, n, k_math<FN>, x, y, out, n);
}

} // namespace

/* fn: the codes above; y is read by pow (element-wise, or y[0] for code 4), ldexp (int32 bits),
   division, min and max, and may be null otherwise. */
DK_API int dk_math(int fn, const float *x, const float *y, float *out, uint32_t n)
{
    if (fn < 0 || fn >= DK_N_MATH) return (int)hipErrorInvalidValue;
    const bool binary = fn == DK_POW || fn >= DK_LDEXP;
    Dev dev;
    const float *dx = dev.in(x, n);
    const float *dy = dev.in(y, binary ? n : (fn == DK_POW_Y0 ? 1u : 0u));
    float *dout = dev.alloc<float>(n);
    switch (fn) {
    case DK_SIN: launch_math<DK_SIN>(dev, dx, dy, dout, n); break;
    case DK_COS: launch_math<DK_COS>(dev, dx, dy, dout, n); break;
    case DK_EXP: launch_math<DK_EXP>(dev, dx, dy, dout, n); break;
    case DK_LOG: launch_math<DK_LOG>(dev, dx, dy, dout, n); break;
    case DK_POW_Y0: launch_math<DK_POW_Y0>(dev, dx, dy, dout, n); break;
    case DK_SINCOS_S: launch_math<DK_SINCOS_S>(dev, dx, dy, dout, n); break;
    case DK_SINCOS_C: launch_math<DK_SINCOS_C>(dev, dx, dy, dout, n); break;
    case DK_POW: launch_math<DK_POW>(dev, dx, dy, dout, n); break;
    case DK_SQRT: launch_math<DK_SQRT>(dev, dx, dy, dout, n); break;
    case DK_RSQRT: launch_math<DK_RSQRT>(dev, dx, dy, dout, n); break;
    case DK_LDEXP: launch_math<DK_LDEXP>(dev, dx, dy, dout, n); break;
    case DK_DIV: launch_math<DK_DIV>(dev, dx, dy, dout, n); break;
    case DK_MIN: launch_math<DK_MIN>(dev, dx, dy, dout, n); break;
    default: launch_math<DK_MAX>(dev, dx, dy, dout, n); break;
    }
    dev.out(out, dout, n);
    return dev.status();
}

/* k draws of frand from each seed pair: vals[n][k] and the seeds after them. */
DK_API int dk_frand(const uint32_t *seeds, uint32_t k, float *vals, uint32_t *seeds_out, uint32_t n)
{
    Dev dev;
    const uint32_t *ds = dev.in(seeds, 2 * (size_t)n);
    float *dv = dev.alloc<float>((size_t)n * k);
    uint32_t *dso = dev.alloc<uint32_t>(2 * (size_t)n);
    DK_LAUNCH(dev, n, k_rand<false>, ds, k, 1, dv, dso, n);
    dev.out(vals, dv, (size_t)n * k);
    dev.out(seeds_out, dso, 2 * (size_t)n);
    return dev.status();
}

/* k draws of strat_rand(seed, j % total, total), j = 0..k-1. */
DK_API int dk_strat_rand(const uint32_t *seeds, uint32_t k, int total, float *vals, uint32_t *seeds_out, uint32_t n)
{
    if (total < 1) return (int)hipErrorInvalidValue;
    Dev dev;
    const uint32_t *ds = dev.in(seeds, 2 * (size_t)n);
    float *dv = dev.alloc<float>((size_t)n * k);
    uint32_t *dso = dev.alloc<uint32_t>(2 * (size_t)n);
    DK_LAUNCH(dev, n, k_rand<true>, ds, k, total, dv, dso, n);
    dev.out(vals, dv, (size_t)n * k);
    dev.out(seeds_out, dso, 2 * (size_t)n);
    return dev.status();
}

/* gen 0: mwc_jump<36969>, gen 1: mwc_jump<18000>. */
DK_API int dk_mwc_jump(int gen, const uint32_t *x, const uint32_t *k, const uint32_t *mul, uint32_t *out, uint32_t n)
{
    Dev dev;
    const uint32_t *dx = dev.in(x, n), *dk = dev.in(k, n), *dm = dev.in(mul, n);
    uint32_t *dout = dev.alloc<uint32_t>(n);
    if (gen == 0) DK_LAUNCH(dev, n, k_mwc_jump<36969u>, dx, dk, dm, dout, n);
    else DK_LAUNCH(dev, n, k_mwc_jump<18000u>, dx, dk, dm, dout, n);
    dev.out(out, dout, n);
    return dev.status();
}

/* hit / t_out: the closest-hit form (t_out = the ray's tmax afterwards); hit_any: the any-hit form. */
DK_API int dk_mt_test(const rt_ray *rays, const rt_triangle *tris, int32_t *hit, float *t_out, int32_t *hit_any,
                      uint32_t n)
{
    Dev dev;
    const rt_ray *dr = dev.in(rays, n);
    const rt_triangle *dt = dev.in(tris, n);
    int32_t *dh = dev.alloc<int32_t>(n), *da = dev.alloc<int32_t>(n);
    float *dto = dev.alloc<float>(n);
    DK_LAUNCH(dev, n, k_mt_test, dr, dt, dh, dto, da, n);
    dev.out(hit, dh, n);
    dev.out(t_out, dto, n);
    dev.out(hit_any, da, n);
    return dev.status();
}

DK_API int dk_intersect_sphere(const rt_ray *rays, const float *c, const float *radius, float *out, uint32_t n)
{
    Dev dev;
    const rt_ray *dr = dev.in(rays, n);
    const float *dc = dev.in(c, 3 * (size_t)n), *drad = dev.in(radius, n);
    float *dout = dev.alloc<float>(n);
    DK_LAUNCH(dev, n, k_sphere, dr, dc, drad, dout, n);
    dev.out(out, dout, n);
    return dev.status();
}

DK_API int dk_intersect_box(const rt_ray *rays, float xs, float ys, float zs, float *t_out, float *nrm, uint32_t n)
{
    Dev dev;
    const rt_ray *dr = dev.in(rays, n);
    float *dt = dev.alloc<float>(n), *dn = dev.alloc<float>(3 * (size_t)n);
    DK_LAUNCH(dev, n, k_box, dr, xs, ys, zs, dt, dn, n);
    dev.out(t_out, dt, n);
    dev.out(nrm, dn, 3 * (size_t)n);
    return dev.status();
}

DK_API int dk_camera_dir(const rt_camera *cams, uint32_t n_cams, const int32_t *cam_idx, const float *a,
                         const float *b, float *out, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i)
        if (cam_idx[i] < 0 || (uint32_t)cam_idx[i] >= n_cams) return (int)hipErrorInvalidValue;
    Dev dev;
    const rt_camera *dc = dev.in(cams, n_cams);
    const int32_t *di = dev.in(cam_idx, n);
    const float *da = dev.in(a, n), *db = dev.in(b, n);
    float *dout = dev.alloc<float>(3 * (size_t)n);
    DK_LAUNCH(dev, n, k_camera_dir, dc, di, da, db, dout, n);
    dev.out(out, dout, 3 * (size_t)n);
    return dev.status();
}

/* fn 0: perpendicular(v); 1: shading_to_world(v, nrm); 2: world_to_shading(v, nrm). */
DK_API int dk_frame(int fn, const float *v, const float *nrm, float *out, uint32_t n)
{
    if (fn < 0 || fn > 2) return (int)hipErrorInvalidValue;
    Dev dev;
    const float *dv = dev.in(v, 3 * (size_t)n);
    const float *dn = dev.in(nrm, fn ? 3 * (size_t)n : 0);
    float *dout = dev.alloc<float>(3 * (size_t)n);
    if (fn == 0) DK_LAUNCH(dev, n, k_frame<0>, dv, dn, dout, n);
    else if (fn == 1) DK_LAUNCH(dev, n, k_frame<1>, dv, dn, dout, n);
    else DK_LAUNCH(dev, n, k_frame<2>, dv, dn, dout, n);
    dev.out(out, dout, 3 * (size_t)n);
    return dev.status();
}

DK_API int dk_cos_sample_hemisphere(const float *r1, const float *r2, float *out, uint32_t n)
{
    Dev dev;
    const float *d1 = dev.in(r1, n), *d2 = dev.in(r2, n);
    float *dout = dev.alloc<float>(3 * (size_t)n);
    DK_LAUNCH(dev, n, k_cos_sample_hemisphere, d1, d2, dout, n);
    dev.out(out, dout, 3 * (size_t)n);
    return dev.status();
}

DK_API int dk_sample_phong(const float *w, const float *spec_exp, const float *r1, const float *r2, float *out,
                           uint32_t n)
{
    Dev dev;
    const float *dw = dev.in(w, 3 * (size_t)n), *de = dev.in(spec_exp, n), *d1 = dev.in(r1, n), *d2 = dev.in(r2, n);
    float *dout = dev.alloc<float>(3 * (size_t)n);
    DK_LAUNCH(dev, n, k_sample_phong, dw, de, d1, d2, dout, n);
    dev.out(out, dout, 3 * (size_t)n);
    return dev.status();
}

/* rays in and out (d and propagation change); ret: the function's return value. */
DK_API int dk_sample_refraction(rt_ray *rays, const float *ior, const float *blur_exp, const float *r1,
                                const float *r2, int32_t *ret, uint32_t n)
{
    Dev dev;
    rt_ray *dr = dev.in(rays, n);
    const float *di = dev.in(ior, n), *db = dev.in(blur_exp, n), *d1 = dev.in(r1, n), *d2 = dev.in(r2, n);
    int32_t *dret = dev.alloc<int32_t>(n);
    DK_LAUNCH(dev, n, k_sample_refraction, dr, di, db, d1, d2, dret, n);
    dev.out(rays, dr, n);
    dev.out(ret, dret, n);
    return dev.status();
}

DK_API int dk_sphere_light_dir(const float *o, const float *c, const float *radius, const float *r1, const float *r2,
                               float *dir, float *tmax, uint32_t n)
{
    Dev dev;
    const float *dor = dev.in(o, 3 * (size_t)n), *dc = dev.in(c, 3 * (size_t)n), *drad = dev.in(radius, n);
    const float *d1 = dev.in(r1, n), *d2 = dev.in(r2, n);
    float *dd = dev.alloc<float>(3 * (size_t)n), *dt = dev.alloc<float>(n);
    DK_LAUNCH(dev, n, k_sphere_light_dir, dor, dc, drad, d1, d2, dd, dt, n);
    dev.out(dir, dd, 3 * (size_t)n);
    dev.out(tmax, dt, n);
    return dev.status();
}

/* rays and seeds in and out; hits: hit point and normal (6 floats); mats[mat_idx[i]] is the material. */
DK_API int dk_sample_material(rt_ray *rays, const float *hits, const rt_material *mats, uint32_t n_mats,
                              const int32_t *mat_idx, uint32_t *seeds, int32_t *ret, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i)
        if (mat_idx[i] < 0 || (uint32_t)mat_idx[i] >= n_mats) return (int)hipErrorInvalidValue;
    Dev dev;
    rt_ray *dr = dev.in(rays, n);
    const float *dh = dev.in(hits, 6 * (size_t)n);
    const rt_material *dm = dev.in(mats, n_mats);
    const int32_t *di = dev.in(mat_idx, n);
    uint32_t *ds = dev.in(seeds, 2 * (size_t)n);
    int32_t *dret = dev.alloc<int32_t>(n);
    DK_LAUNCH(dev, n, k_sample_material, dr, dh, dm, di, ds, dret, n);
    dev.out(rays, dr, n);
    dev.out(seeds, ds, 2 * (size_t)n);
    dev.out(ret, dret, n);
    return dev.status();
}
