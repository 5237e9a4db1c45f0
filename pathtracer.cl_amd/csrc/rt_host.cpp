/*
 * rt_host.cpp — the C-ABI host runtime (librtmi.so), MI355X replacement of
 * the reference's OpenCL host RayTracerCL (clrt/RayTracerCL.cpp) and of the
 * device-agnostic RayTracer settings (clrt/RayTracer.cpp).
 *
 * This file: the context's life (rt_create / rt_destroy), the scene's spheres, the camera
 * derivation, the settings and the seed planes.  The mesh is rt_mesh.cpp's, the renders
 * rt_render.cpp's, the display-side stages rt_display.cpp's; the context itself is rt_ctx.h.
 * There is no CPU fallback: every render runs the HIP kernels or returns an error.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>

#include "rt_ctx.h"
#include "rt_math.h"

/* glibc random() TYPE_3 (the generator behind rand(), seeded with 1 when the
   program never calls srand — the reference never does).  Published algorithm:
   r[0] = seed; r[i] = 16807 r[i-1] mod (2^31-1) for i < 31; r[i] = r[i-31]
   for 31 <= i < 34; then r[i] = r[i-31] + r[i-3] (mod 2^32) and the outputs
   are r[i] >> 1 from i = 344 on. */
void GlibcRand::seed(uint32_t s)
{
    int32_t w[344 + 34];
    if (s == 0) s = 1;
    w[0] = (int32_t)s;
    for (int i = 1; i < 31; ++i) {
        const int64_t v = (16807LL * w[i - 1]) % 2147483647LL;
        w[i] = (int32_t)(v < 0 ? v + 2147483647LL : v);
    }
    for (int i = 31; i < 34; ++i) w[i] = w[i - 31];
    uint32_t u[344];
    for (int i = 0; i < 34; ++i) u[i] = (uint32_t)w[i];
    for (int i = 34; i < 344; ++i) u[i] = u[i - 31] + u[i - 3];
    for (int i = 0; i < 34; ++i) r[i] = u[310 + i]; /* last 34 values, oldest first */
    k = 0;
}

uint32_t GlibcRand::next()
{
    /* r holds the last 34 values in a ring starting at k (oldest) */
    const uint32_t v = r[(k + 34 - 31) % 34] + r[(k + 34 - 3) % 34];
    r[k] = v;
    k = (k + 1) % 34;
    return v >> 1;
}

namespace {

constexpr double kPi = 3.14159265358979323846; /* M_PI */

/* RayTracer::setCameraSpherical (RayTracer.cpp:33-47): gmtl EulerAngle<ZYX>
   (0, yaw, pitch) -> quaternion qz*qy*qx (Generate.h:214-260), normalised
   (QuatOps.h:337-351), position = q (0,0,d) q* (Xforms.h:40-60) + target, and
   the rotation matrix of q (Generate.h:1143-1176).  float arithmetic in gmtl's
   order; the two angle conversions are binary64 as in the D2R macro. */
void spherical_view(float tx, float ty, float tz, float el, float az, float dist, float m[4][4])
{
    const float yaw = (float)(-(az * kPi / 180.0f) + kPi);
    const float pitch = (float)(-(el * kPi / 180.0f));
    const float xr = pitch, yr = yaw, zr = 0.0f;
    const float x2 = xr * 0.5f, y2 = yr * 0.5f, z2 = zr * 0.5f;
    /* quaternions as (x, y, z, w) */
    const float qx[4] = {std::sin(x2), 0.0f, 0.0f, std::cos(x2)};
    const float qy[4] = {0.0f, std::sin(y2), 0.0f, std::cos(y2)};
    const float qz[4] = {0.0f, 0.0f, std::sin(z2), std::cos(z2)};
    auto qmul = [](const float *a, const float *b, float *r) {
        r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
        r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
        r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
        r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    };
    float t[4], q[4];
    qmul(qz, qy, t);
    qmul(t, qx, q);
    const float len = std::sqrt((((q[0] * q[0]) + (q[1] * q[1])) + (q[2] * q[2])) + (q[3] * q[3]));
    if (!(len < 0.0001f)) {
        const float li = 1.0f / len;
        for (int i = 0; i < 4; ++i) q[i] *= li;
    }
    /* position = q * (0,0,dist) * conj(q) */
    const float rc[4] = {-q[0], -q[1], -q[2], q[3]};
    const float pure[4] = {0.0f, 0.0f, dist, 0.0f};
    float tmp[4];
    tmp[0] = pure[3] * rc[0] + pure[0] * rc[3] + pure[1] * rc[2] - pure[2] * rc[1];
    tmp[1] = pure[3] * rc[1] + pure[1] * rc[3] + pure[2] * rc[0] - pure[0] * rc[2];
    tmp[2] = pure[3] * rc[2] + pure[2] * rc[3] + pure[0] * rc[1] - pure[1] * rc[0];
    tmp[3] = pure[3] * rc[3] - pure[0] * rc[0] - pure[1] * rc[1] - pure[2] * rc[2];
    const float px = q[3] * tmp[0] + q[0] * tmp[3] + q[1] * tmp[2] - q[2] * tmp[1];
    const float py = q[3] * tmp[1] + q[1] * tmp[3] + q[2] * tmp[0] - q[0] * tmp[2];
    const float pz = q[3] * tmp[2] + q[2] * tmp[3] + q[0] * tmp[1] - q[1] * tmp[0];
    /* rotation part (Watt & Watt) */
    const float xs = q[0] + q[0], ys = q[1] + q[1], zs = q[2] + q[2];
    const float xx = q[0] * xs, xy = q[0] * ys, xz = q[0] * zs;
    const float yy = q[1] * ys, yz = q[1] * zs, zz = q[2] * zs;
    const float wx = q[3] * xs, wy = q[3] * ys, wz = q[3] * zs;
    m[0][0] = 1.0f - (yy + zz);
    m[1][0] = xy + wz;
    m[2][0] = xz - wy;
    m[0][1] = xy - wz;
    m[1][1] = 1.0f - (xx + zz);
    m[2][1] = yz + wx;
    m[0][2] = xz + wy;
    m[1][2] = yz - wx;
    m[2][2] = 1.0f - (xx + yy);
    m[3][0] = m[3][1] = m[3][2] = 0.0f;
    m[3][3] = 1.0f;
    m[0][3] = px + tx;
    m[1][3] = py + ty;
    m[2][3] = pz + tz;
}

/* RayTracerCL::updateCLCamera (RayTracerCL.cpp:178-215). */
void camera_from_view(const float m[4][4], float fov_deg, uint32_t width, rt_camera *c)
{
    auto xform = [&](float v0, float v1, float v2, float *r) { /* gmtl Matrix44 * Vec3 (w = 0), Xforms.h:113-190 */
        float res[4];
        for (int i = 0; i < 4; ++i) {
            res[i] = 0.0f;
            res[i] += m[i][0] * v0;
            res[i] += m[i][1] * v1;
            res[i] += m[i][2] * v2;
            res[i] += m[i][3] * 0.0f;
        }
        if (!(std::fabs(res[3] - 0.0f) <= 0.0001f)) {
            const float wi = 1.0f / res[3];
            for (int i = 0; i < 3; ++i) r[i] = res[i] * wi;
        } else {
            for (int i = 0; i < 3; ++i) r[i] = res[i];
        }
    };
    float view[3], up[3], right[3];
    xform(0.0f, 0.0f, -1.0f, view);
    xform(0.0f, 1.0f, 0.0f, up);
    right[0] = (view[1] * up[2]) - (view[2] * up[1]);
    right[1] = (view[2] * up[0]) - (view[0] * up[2]);
    right[2] = (view[0] * up[1]) - (view[1] * up[0]);
    const float s = (float)((width / 2.0) / std::tan((fov_deg * kPi / 180.0f) / 2.0));
    for (int i = 0; i < 3; ++i) view[i] *= s;
    c->view = {view[0], view[1], view[2], 0.0f};
    c->up = {up[0], up[1], up[2], 0.0f};
    c->right = {right[0], right[1], right[2], 0.0f};
    c->position = {m[0][3], m[1][3], m[2][3], 0.0f};
}

} // namespace

rt_camera frame_camera(const rt_ctx *c, uint32_t W)
{
    rt_camera cam;
    if (c->cam_override) cam = c->cam_explicit;
    else camera_from_view(c->view, c->fov, W, &cam);
    return cam;
}

int ensure_seeds(rt_ctx *c, uint32_t wpad, uint32_t hpad, const uint32_t *src)
{
    const size_t count = 2ull * wpad * hpad;
    if (wpad != c->wpad || hpad != c->hpad) {
        c->d_seeds.reset(); /* (a new layout, larger or smaller: not grow-only) */
        c->wpad = c->hpad = 0;
        if (count) HIPCHK(c, c->d_seeds.reserve(count));
        c->wpad = wpad;
        c->hpad = hpad;
    }
    std::vector<uint32_t> host;
    if (!src) { /* RayTracerCL::updateSeedBuffer: rand(), values < 2 raised to 2 */
        host.resize(count);
        for (size_t i = 0; i < count; ++i) {
            uint32_t v = c->rng.next();
            host[i] = v < 2 ? 2 : v;
        }
        src = host.data();
    }
    if (count) HIPCHK(c, hipMemcpy(c->d_seeds, src, count * sizeof(uint32_t), hipMemcpyHostToDevice));
    return RT_OK;
}

int rt_exception_status(std::string *err) noexcept
{
    int code = RT_ERR_STATE;
    const char *what = "unknown exception";
    try {
        throw;
    } catch (const std::bad_alloc &e) {
        code = RT_ERR_ALLOC;
        what = e.what();
    } catch (const std::length_error &e) {
        code = RT_ERR_ALLOC;
        what = e.what();
    } catch (const std::exception &e) {
        code = RT_ERR_ARG;
        what = e.what();
    } catch (...) {
    }
    if (err) {
        try {
            *err = std::string("host exception: ") + what;
        } catch (...) {
        }
    }
    return code;
}

extern "C" {

const char *rt_status_string(int s)
{
    switch (s) {
    case RT_OK: return "ok";
    case RT_ERR_ARG: return "invalid argument";
    case RT_ERR_HIP: return "HIP runtime error";
    case RT_ERR_NO_SCENE: return "no spheres set";
    case RT_ERR_NO_MESH: return "no mesh set";
    case RT_ERR_ALLOC: return "allocation failed";
    case RT_ERR_STATE: return "invalid state";
    case RT_ERR_LIMIT: return "device limit exceeded";
    default: return "unknown status";
    }
}

int rt_create(int device, rt_ctx **out)
try {
    if (!out) return RT_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return RT_ERR_HIP;
    if (device < 0 || device >= n) return RT_ERR_ARG;
    rt_ctx *c = new (std::nothrow) rt_ctx();
    if (!c) return RT_ERR_ALLOC;
    c->device = device;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) c->view[i][j] = (i == j) ? 1.0f : 0.0f;
    c->rng.seed(1);
    /* A/B and capacity knobs (none changes a result bit) */
    if (const char *sch = getenv("RT_SCHEDULE")) c->schedule = std::string(sch) != "0";
    if (const char *v = getenv("RT_SPLIT_MB")) c->split_mb = (size_t)std::max(0L, atol(v));
    if (const char *v = getenv("RT_SPLIT")) c->split = atoi(v) != 0 ? 1 : 0;
    if (const char *v = getenv("RT_SPLIT_SPEC")) c->split_spec = atoi(v);
    if (const char *v = getenv("RT_SEED_WIDTH")) { /* test knob: 0 automatic, 1 one lane, 3 cooperative, 8-64 (a power of two) */
        const int w = atoi(v);
        if (w == 0 || w == 1 || w == 3 || (w >= 8 && w <= 64 && (w & (w - 1)) == 0)) c->seed_width = (uint32_t)w;
        else fprintf(stderr, "[rtmi] RT_SEED_WIDTH=%s ignored (0, 1, 3 or a power of two from 8 to 64)\n", v);
    }
    if (const char *v = getenv("RT_PIXEL_LISTS")) c->pixel_lists = atoi(v) != 0 ? 1 : 0;
    if (const char *v = getenv("RT_PILOT")) c->pilot_sr = std::max(0, std::min(8, atoi(v))); /* test knob */
    c->repair_slots = std::max(1u, env_u32("RT_REPAIR_SLOTS", RT_REPAIR_SLOTS)); /* test knob: the path beyond them */
    if (const char *v = getenv("RT_LIST_MB")) c->list_mb = (size_t)std::max(0L, atol(v));
    if (const char *v = getenv("RT_SHADOW_CACHE")) c->shadow_cache = atoi(v) != 0;
    if (const char *v = getenv("RT_SHADOW_CACHE_DEPTH")) c->shadow_cache_depth = std::max(0, atoi(v));
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        c->ev0.create() != hipSuccess || c->ev1.create() != hipSuccess || c->evm.create() != hipSuccess ||
        c->ev_done.create(hipEventDisableTiming) != hipSuccess ||
        c->d_totals.reserve(RT_COUNTER_WORDS + 1) != hipSuccess ||
        hipMemset(c->d_totals, 0, (RT_COUNTER_WORDS + 1) * sizeof(unsigned long long)) != hipSuccess ||
        c->d_counters.reserve((kCounterBytes + kWorkWords * sizeof(uint32_t)) / sizeof(unsigned long long)) != hipSuccess ||
        hipHostMalloc(&c->h_counters, kCounterBytes + sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
        rt_destroy(c);
        return RT_ERR_HIP;
    }
    memset(c->h_counters, 0, kCounterBytes + sizeof(unsigned long long)); /* no stale guard before any render */
    c->d_work = reinterpret_cast<uint32_t *>(c->d_counters + RT_COUNTER_WORDS);
    /* the pinned copy's device address: a render hands its counters back with k_counters_out (a copy-engine
       transfer where the mapping is unavailable) */
    void *hd = nullptr;
    if (hipHostGetDevicePointer(&hd, c->h_counters, 0) == hipSuccess)
        c->h_counters_dev = static_cast<unsigned long long *>(hd);
    *out = c;
    return RT_OK;
} RT_CATCH(nullptr)

/* What has an order: the context's stream drained and a pending display-side call ended before
   anything is freed; the members free themselves (rt_ctx.h). */
int rt_destroy(rt_ctx *c)
try {
    if (!c) return RT_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->aux_stream) (void)hipEventSynchronize(c->ev_aux);
    delete c;
    return RT_OK;
} RT_CATCH(err_of(c))

const char *rt_last_error(const rt_ctx *c) { return c ? c->err.c_str() : "null context"; }

int rt_set_spheres(rt_ctx *c, const rt_sphere *s, uint32_t n)
try {
    if (!c || (n && !s)) return RT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    c->spheres.assign(s, s + n);
    c->lights.clear();
    for (uint32_t i = 0; i < n; ++i)
        if (s[i].mat.emission_power != 0) c->lights.push_back(s[i]); /* rtcommon.h:90 */
    c->d_spheres.reset();
    c->d_lights.reset();
    if (n) {
        HIPCHK(c, c->d_spheres.reserve(n));
        HIPCHK(c, hipMemcpy(c->d_spheres, s, n * sizeof(rt_sphere), hipMemcpyHostToDevice));
    }
    if (!c->lights.empty()) {
        HIPCHK(c, c->d_lights.reserve(c->lights.size()));
        HIPCHK(c, hipMemcpy(c->d_lights, c->lights.data(), c->lights.size() * sizeof(rt_sphere),
                            hipMemcpyHostToDevice));
    }
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_set_view_matrix(rt_ctx *c, const float m[16])
try {
    if (!c || !m) return RT_ERR_ARG;
    for (int col = 0; col < 4; ++col)
        for (int row = 0; row < 4; ++row) c->view[row][col] = m[col * 4 + row];
    c->cam_override = false;
    c->cam_dirty = true;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_set_camera_spherical(rt_ctx *c, float tx, float ty, float tz, float el, float az, float dist)
try {
    if (!c) return RT_ERR_ARG;
    spherical_view(tx, ty, tz, el, az, dist, c->view);
    c->cam_override = false;
    c->cam_dirty = true;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_set_fov(rt_ctx *c, float fov)
try {
    if (!c) return RT_ERR_ARG;
    c->fov = fov;
    c->cam_override = false;
    c->cam_dirty = true;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_set_camera(rt_ctx *c, const rt_camera *cam)
try {
    if (!c || !cam) return RT_ERR_ARG;
    c->cam_explicit = *cam;
    c->cam_override = true;
    c->cam_dirty = true;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_camera_spherical(float tx, float ty, float tz, float el, float az, float dist, float fov, uint32_t width,
                        rt_camera *out)
try {
    if (!out) return RT_ERR_ARG;
    float m[4][4];
    spherical_view(tx, ty, tz, el, az, dist, m);
    camera_from_view(m, fov, width, out);
    return RT_OK;
} RT_CATCH(nullptr)

int rt_set_params(rt_ctx *c, uint32_t sample_rate, uint32_t max_depth)
try {
    if (!c) return RT_ERR_ARG;
    if (sample_rate > 4096) return fail(c, RT_ERR_ARG, "sample rate too large");
    c->sample_rate = sample_rate;
    c->max_depth = max_depth;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_set_builder(rt_ctx *c, int builder)
try {
    if (!c || (builder != RT_BUILD_HOST && builder != RT_BUILD_GPU && builder != RT_BUILD_GPU_PLOC)) return RT_ERR_ARG;
    c->builder = builder;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_set_build_options(rt_ctx *c, uint32_t opts)
try {
    if (!c) return RT_ERR_ARG;
    if (opts & ~(uint32_t)RT_BUILD_OPT_LIGHTS) return fail(c, RT_ERR_ARG, "rt_set_build_options: unknown option bits");
    c->build_opts = opts;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_get_build_options(const rt_ctx *c, uint32_t *opts)
try {
    if (!c || !opts) return RT_ERR_ARG;
    *opts = c->build_opts;
    return RT_OK;
} RT_CATCH(nullptr)

int rt_set_collapse(rt_ctx *c, int mode)
try {
    if (!c) return RT_ERR_ARG;
    if (mode != RT_COLLAPSE_GREEDY && mode != RT_COLLAPSE_SAH) return fail(c, RT_ERR_ARG, "rt_set_collapse: unknown mode");
    c->collapse = mode;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_get_collapse(const rt_ctx *c, int *mode)
try {
    if (!c || !mode) return RT_ERR_ARG;
    *mode = c->collapse;
    return RT_OK;
} RT_CATCH(nullptr)

int rt_set_traversal(rt_ctx *c, int t)
try {
    if (!c || !(t == RT_TRAVERSAL_BVH || t == RT_TRAVERSAL_LINEAR || t == RT_TRAVERSAL_BVH4F)) return RT_ERR_ARG;
    c->traversal = t;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_set_ndrange(rt_ctx *c, uint32_t nd_y)
try {
    if (!c || nd_y == 0 || nd_y > 1024) return RT_ERR_ARG;
    c->nd_y = nd_y;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_set_seed_layout(rt_ctx *c, uint32_t wpad, uint32_t hpad)
try {
    if (!c || !wpad || !hpad) return RT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int r = ensure_seeds(c, wpad, hpad, nullptr);
    if (r == RT_OK) c->user_seeds = true;
    return r;
} RT_CATCH(err_of(c))

int rt_set_seeds(rt_ctx *c, const uint32_t *seeds, size_t count)
try {
    if (!c || !seeds) return RT_ERR_ARG;
    if (!c->wpad || count != 2ull * c->wpad * c->hpad) return fail(c, RT_ERR_STATE, "seed count != 2*Wpad*Hpad");
    HIPCHK(c, hipSetDevice(c->device));
    const int r = ensure_seeds(c, c->wpad, c->hpad, seeds);
    if (r == RT_OK) c->user_seeds = true;
    return r;
} RT_CATCH(err_of(c))

int rt_get_seeds(const rt_ctx *c, uint32_t *out, size_t count)
try {
    if (!c || !out) return RT_ERR_ARG;
    if (!c->wpad || count != 2ull * c->wpad * c->hpad) return RT_ERR_STATE;
    if (hipSetDevice(c->device) != hipSuccess) return RT_ERR_HIP;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return RT_ERR_HIP;
    if (hipMemcpy(out, c->d_seeds, count * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return RT_ERR_HIP;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_seed_layout(const rt_ctx *c, uint32_t *wpad, uint32_t *hpad)
try {
    if (!c) return RT_ERR_ARG;
    if (wpad) *wpad = c->wpad;
    if (hpad) *hpad = c->hpad;
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_glibc_rand_fill(uint32_t seed, uint32_t *out, size_t count, uint32_t skip)
try {
    if (!out && count) return RT_ERR_ARG;
    GlibcRand g;
    g.seed(seed);
    for (uint32_t i = 0; i < skip; ++i) (void)g.next();
    for (size_t i = 0; i < count; ++i) out[i] = g.next();
    return RT_OK;
} RT_CATCH(nullptr)

int rt_get_camera(const rt_ctx *c, uint32_t width, rt_camera *out)
try {
    if (!c || !out || width == 0) return RT_ERR_ARG;
    *out = frame_camera(c, width);
    return RT_OK;
} RT_CATCH(err_of(c))

int rt_primary_rays(const rt_camera *cam, uint32_t W, uint32_t H, rt_ray *out)
try {
    if (!cam || !out || W == 0 || H == 0) return RT_ERR_ARG;
    const float hw = ((float)W) / 2.0f, hh = ((float)H) / 2.0f;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            /* the kernels' camera_dir (raytracer.cl:81-85): float4 lanes incl. w, v / sqrt(dot(v, v)) */
            const float a = ((float)x + 0.5f) - hw, b = ((float)y + 0.5f) - hh;
            const float vx = (cam->view.x + cam->right.x * a) + cam->up.x * b;
            const float vy = (cam->view.y + cam->right.y * a) + cam->up.y * b;
            const float vz = (cam->view.z + cam->right.z * a) + cam->up.z * b;
            const float vw = (cam->view.w + cam->right.w * a) + cam->up.w * b;
            const float len = rt_sqrtf(((vx * vx + vy * vy) + vz * vz) + vw * vw);
            rt_ray &r = out[(size_t)y * W + x];
            r.o = {cam->position.x, cam->position.y, cam->position.z};
            r.d = {vx / len, vy / len, vz / len};
            r.tmin = RT_SMALL_F;
            r.tmax = rt_inff();
            r.propagation = {1.0f, 1.0f, 1.0f};
            r.extinction = {0.0f, 0.0f, 0.0f};
            r.diffuse_bounce = 0;
        }
    return RT_OK;
} RT_CATCH(nullptr)

} /* extern "C" */
