/*
 * rt_lists.hip — the camera-ray candidate lists: a pre-pass per view that gives every pixel the
 * few triangles any of its camera rays could accept, which k_tris and the seed passes then test
 * instead of walking the tree (RtTriLaunch::list_code in rt_internal.h, list_pack in
 * rt_kernel_util.h).
 *
 *   Frustum, pixel_dir_box, pixel_square, frustum_slab, frustum_det, tri_padded_box,
 *   tri_meets_pixel       a pixel's rays as a direction box and a square, and the conservative
 *                         tests of boxes and triangles against them, all in binary64
 *   frustum_list          the conservative traversal (not inlined: k_pixel_lists is its only caller)
 *   k_pixel_lists         one wave per 8 x 8 tile: the lists, ranked by earliest accept, in one
 *                         block of the list area
 *   rt_launch_pixel_lists
 *
 * Culling only, and off the render loop: nothing here is shared with the other kernels but
 * camera_dir and global_row.
 */
#include <hip/hip_runtime.h>

#include "rt_device.h"
#include "rt_internal.h"
#include "rt_quant.h"
#include "rt_traverse.h"
#include "rt_kernel_util.h"

#pragma clang fp contract(off)

namespace {

/* Camera-ray candidate lists.  A pixel's sampleRate^2 camera rays share the camera position
   and leave through the pixel's square (strat_rand offsets in [0, 1], raytracer.cl:216-224), so
   one conservative traversal of that narrow frustum finds every triangle any of them could
   accept: directions bounded component-wise by the four corner rays (camera_dir, the kernel's
   own arithmetic) padded by 1e-5; boxes tested with interval slabs in binary64 (per axis the
   earliest entry and latest exit over the direction interval — a necessary condition for a
   hit); nodes whose normal box keeps |d . N| below the determinant threshold for every
   direction skipped (rt_quant.h); triangles kept if their padded box (the builder's pad) meets
   the frustum and some direction could give |det| >= 1e-4 (with det's float error).  Up to
   RT_LIST_MAX survivors are copied into the pixel's list slots; k_tris then answers each camera
   query by testing only them (a virtual leaf: the same tests and accept rule on the same
   records, so the same closest hit), and an empty list answers "no mesh hit" outright.  Pixels
   with more candidates (or a stack overflow) keep the BVH. */
struct Frustum {
    double o[3];           /* the rays' origin (the camera) */
    double dlo[3], dhi[3]; /* their directions (component-wise interval) */
    double ilo[3], ihi[3]; /* 1 / dlo, 1 / dhi */
    double l1;             /* max |d|_1 */
    /* the pixel in the camera's own coordinates: P - o = s0 view + s1 right + s2 up (minv: that
       basis inverted), a ray of the pixel through P has a = s1 / s0 in [a0, a1], b = s2 / s0 in
       [b0, b1] (pixel_square); proj false: no such test */
    double minv[9];
    double a0, a1, b0, b1;
    bool proj;
};

/* The pixel's square in the camera's (a, b) coordinates, padded for the float evaluation of
   camera_dir: its rays are o + t (view + right a + up b) exactly for a in [ax, ax + 1], b in
   [by, by + 1] (the strat_rand offsets, raytracer.cl:216-224; the subtraction of W / 2 is exact),
   and the float direction strays from that ray by a few ulp of |view| + |right a| + |up b|,
   which moves (a, b) by that over |right| or |up| plus (|a| + |b|) times it over |view|: the pad
   covers it 20 times over. */
__device__ __forceinline__ void pixel_square(Frustum &f, const rt_camera &cam, float ax, float by)
{
    const double c[3][3] = {{cam.view.x, cam.right.x, cam.up.x}, {cam.view.y, cam.right.y, cam.up.y},
                            {cam.view.z, cam.right.z, cam.up.z}};
    const double det = c[0][0] * (c[1][1] * c[2][2] - c[1][2] * c[2][1]) - c[0][1] * (c[1][0] * c[2][2] - c[1][2] * c[2][0]) +
                       c[0][2] * (c[1][0] * c[2][1] - c[1][1] * c[2][0]);
    const double nv = sqrt(c[0][0] * c[0][0] + c[1][0] * c[1][0] + c[2][0] * c[2][0]);
    const double nr = sqrt(c[0][1] * c[0][1] + c[1][1] * c[1][1] + c[2][1] * c[2][1]);
    const double nu = sqrt(c[0][2] * c[0][2] + c[1][2] * c[1][2] + c[2][2] * c[2][2]);
    f.proj = fabs(det) > 1e-6 * nv * nr * nu && fmin(nr, nu) > 0.0 &&
             (double)cam.view.w == 0.0 && (double)cam.right.w == 0.0 && (double)cam.up.w == 0.0;
    if (!f.proj) return;
    const double id = 1.0 / det;
    f.minv[0] = (c[1][1] * c[2][2] - c[1][2] * c[2][1]) * id;
    f.minv[1] = (c[0][2] * c[2][1] - c[0][1] * c[2][2]) * id;
    f.minv[2] = (c[0][1] * c[1][2] - c[0][2] * c[1][1]) * id;
    f.minv[3] = (c[1][2] * c[2][0] - c[1][0] * c[2][2]) * id;
    f.minv[4] = (c[0][0] * c[2][2] - c[0][2] * c[2][0]) * id;
    f.minv[5] = (c[0][2] * c[1][0] - c[0][0] * c[1][2]) * id;
    f.minv[6] = (c[1][0] * c[2][1] - c[1][1] * c[2][0]) * id;
    f.minv[7] = (c[0][1] * c[2][0] - c[0][0] * c[2][1]) * id;
    f.minv[8] = (c[0][0] * c[1][1] - c[0][1] * c[1][0]) * id;
    const double mag = nv + nr * (fabs((double)ax) + 1.0) + nu * (fabs((double)by) + 1.0);
    const double pad = 0.01 + 64.0 * 0x1p-24 * mag * (1.0 / fmin(nr, nu) + (fabs((double)ax) + fabs((double)by) + 2.0) / nv);
    f.a0 = (double)ax - pad;
    f.a1 = (double)ax + 1.0 + pad;
    f.b0 = (double)by - pad;
    f.b1 = (double)by + 1.0 + pad;
}

/* Can a camera ray of the pixel meet the triangle v0 + u e1 + v e2 (the record's float values, as
   mt_test reads them) where the float test could accept?  The triangle is widened to u, v >= -eps,
   u + v <= 1 + 2 eps, eps bounding the float test's barycentric error (a few ulp of |e| |o - v0|
   and |e1| |e2| over |det| >= 1e-4, 7x margin), projected through the camera onto the pixel's
   (a, b) plane, and tested against the padded square by separating axes (the square's two and the
   triangle's three edge normals).  A vertex at or behind the camera's plane keeps the triangle.
   Culling only; false means no ray of the pixel can accept it. */
__device__ __forceinline__ bool tri_meets_pixel(const Frustum &f, float4 r0, float4 r1, float4 r2, double dist)
{
    if (!f.proj) return true;
    const double e1[3] = {r1.x, r1.y, r1.z}, e2[3] = {r2.x, r2.y, r2.z};
    const double n1 = fabs(e1[0]) + fabs(e1[1]) + fabs(e1[2]), n2 = fabs(e2[0]) + fabs(e2[1]) + fabs(e2[2]);
    const double eps = 8.0 * 16.0 * 0x1p-24 * ((n1 + n2) * dist + n1 * n2) / 1e-4 + 1e-6;
    const double uv[3][2] = {{-eps, -eps}, {1.0 + 3.0 * eps, -eps}, {-eps, 1.0 + 3.0 * eps}};
    double pa[3], pb[3];
    for (int i = 0; i < 3; ++i) {
        double q[3];
        for (int k = 0; k < 3; ++k)
            q[k] = ((double)(k == 0 ? r0.x : k == 1 ? r0.y : r0.z) + uv[i][0] * e1[k] + uv[i][1] * e2[k]) - f.o[k];
        const double s0 = f.minv[0] * q[0] + f.minv[1] * q[1] + f.minv[2] * q[2];
        const double s1 = f.minv[3] * q[0] + f.minv[4] * q[1] + f.minv[5] * q[2];
        const double s2 = f.minv[6] * q[0] + f.minv[7] * q[1] + f.minv[8] * q[2];
        if (!(s0 > 1e-9 * (fabs(s1) + fabs(s2) + fabs(s0)))) return true; /* at or behind the camera's plane */
        pa[i] = s1 / s0;
        pb[i] = s2 / s0;
    }
    if (fmax(pa[0], fmax(pa[1], pa[2])) < f.a0 || fmin(pa[0], fmin(pa[1], pa[2])) > f.a1) return false;
    if (fmax(pb[0], fmax(pb[1], pb[2])) < f.b0 || fmin(pb[0], fmin(pb[1], pb[2])) > f.b1) return false;
    const double cx[4] = {f.a0, f.a1, f.a0, f.a1}, cy[4] = {f.b0, f.b0, f.b1, f.b1};
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        double nx = -(pb[j] - pb[i]), ny = pa[j] - pa[i];
        if (nx * (pa[k] - pa[i]) + ny * (pb[k] - pb[i]) < 0.0) {
            nx = -nx;
            ny = -ny;
        }
        bool out = true;
        for (int q = 0; q < 4 && out; ++q) out = nx * (cx[q] - pa[i]) + ny * (cy[q] - pb[i]) < 0.0;
        if (out) return false;
    }
    return true;
}

__device__ __forceinline__ void frustum_init(Frustum &f)
{
    f.l1 = 0.0;
    for (int k = 0; k < 3; ++k) {
        f.ilo[k] = 1.0 / f.dlo[k];
        f.ihi[k] = 1.0 / f.dhi[k];
        f.l1 += fmax(fabs(f.dlo[k]), fabs(f.dhi[k]));
    }
}

__device__ __forceinline__ bool frustum_slab(const Frustum &f, const double lo[3], const double hi[3],
                                             double *tin_out = nullptr)
{
    /* rays o + t d with d in [dlo, dhi]: per axis (P - o) / d is monotonic in d (of one sign), so
       its range is spanned by the two end quotients (as products with the reciprocals: a
       relative 1e-16 against boxes padded by 1e-6 and more) */
    double tin = -1e300, tout = 1e300;
    for (int k = 0; k < 3; ++k) {
        const double a = f.dlo[k], b = f.dhi[k], o = f.o[k];
        if (!(a > 0.0 || b < 0.0)) {
            /* d straddles 0 on this axis: at t >= 0 the rays' coordinate spans
               [o + t a, o + t b], which must reach [lo, hi] (a lower bound on t) */
            if (a < 0.0) tin = fmax(tin, (hi[k] - o) * f.ilo[k]);
            else if (o > hi[k]) return false;
            if (b > 0.0) tin = fmax(tin, (lo[k] - o) * f.ihi[k]);
            else if (o < lo[k]) return false;
            continue;
        }
        const double ne = (a > 0.0 ? lo[k] : hi[k]) - o, fa = (a > 0.0 ? hi[k] : lo[k]) - o;
        const double ia = f.ilo[k], ib = f.ihi[k];
        tin = fmax(tin, fmin(ne * ia, ne * ib));
        tout = fmin(tout, fmax(fa * ia, fa * ib));
    }
    tin = fmax(tin, -1e-3); /* accepted hits have t > tmin > 0 */
    if (tin_out) *tin_out = tin;
    return tin <= tout;
}

/* max over the direction box of |d . n| for n in [nlo, nhi] */
__device__ __forceinline__ double frustum_det(const double dlo[3], const double dhi[3], const double nlo[3],
                                              const double nhi[3])
{
    double mx = 0.0, mn = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double c0 = dlo[k] * nlo[k], c1 = dlo[k] * nhi[k], c2 = dhi[k] * nlo[k], c3 = dhi[k] * nhi[k];
        mx += fmax(fmax(c0, c1), fmax(c2, c3));
        mn += fmin(fmin(c0, c1), fmin(c2, c3));
    }
    return fmax(mx, -mn);
}

/* The builder's padded triangle box (rt_bvh.cpp: extent / 512 + 1e-6 (1 + |coord|), doubled
   here), from a record's vertices, and the largest |N| component of its normal e2 x e1. */
__device__ __forceinline__ void tri_padded_box(float4 r0, float4 r1, float4 r2, double lo[3], double hi[3],
                                               double &nmax)
{
    const float vx[3] = {r0.x, r0.x + r1.x, r0.x + r2.x}, vy[3] = {r0.y, r0.y + r1.y, r0.y + r2.y},
                vz[3] = {r0.z, r0.z + r1.z, r0.z + r2.z};
    const float *vv[3] = {vx, vy, vz};
    float bl[3], bh[3], mabs = 0.0f;
    for (int q = 0; q < 3; ++q) {
        bl[q] = fminf(vv[q][0], fminf(vv[q][1], vv[q][2]));
        bh[q] = fmaxf(vv[q][0], fmaxf(vv[q][1], vv[q][2]));
        mabs = fmaxf(mabs, fmaxf(fabsf(bl[q]), fabsf(bh[q])));
    }
    const float ext = fmaxf(bh[0] - bl[0], fmaxf(bh[1] - bl[1], bh[2] - bl[2]));
    const double pad = 2.0 * ((double)ext * (1.0 / 512.0) + 1e-6 * (1.0 + mabs));
    for (int q = 0; q < 3; ++q) {
        lo[q] = bl[q] - pad;
        hi[q] = bh[q] + pad;
    }
    const double e1[3] = {r1.x, r1.y, r1.z}, e2[3] = {r2.x, r2.y, r2.z};
    nmax = fmax(fabs(e2[1] * e1[2] - e2[2] * e1[1]),
                fmax(fabs(e2[2] * e1[0] - e2[0] * e1[2]), fabs(e2[0] * e1[1] - e2[1] * e1[0])));
}

/* the pre-pass's per-lane traversal stack, in LDS (it was 256 B of scratch per lane): 48 entries
   cover a 4-wide tree of depth 15 (the dragon needs 35); deeper, the pixel takes the tree */
constexpr int kFrustumStack = 48;

__device__ bool frustum_list(const float *__restrict__ nodes4, const uint32_t *__restrict__ q4,
                             const float4 *__restrict__ tris, const Frustum &f, int *slots, float *keys, uint32_t cap,
                             uint32_t &n, lds_int *stack);

/* The component-wise box of the unit directions normalize(view + right a + up b) over a pixel's
   square a in [ax, ax + 1], b in [by, by + 1] (strat_rand offsets, raytracer.cl:216-224).  The
   four corner rays (camera_dir, the kernel's own float arithmetic) span it only up to the
   curvature of the normalisation: an interior direction leaves the corners' box by about
   1 / (8 L^2), L = (W / 2) / tan(fov / 2) (2e-5 at W = 64).  Bound: d = v / |v| has
   |D^2 d[w, w]| <= 6 |w|^2 / |v|^2, and a C^2 function on the unit square differs from the
   bilinear interpolation of its corners (whose range is the corners' box) by at most
   (1/8)(max |d_aa| + max |d_bb|) = 0.75 (|right|^2 + |up|^2) / min|v|^2, with min|v| over the
   square at least the smallest corner |v| less |right| + |up|.  The pad on top covers the
   float evaluation of camera_dir (a few ulp of a unit vector). */
__device__ __forceinline__ void pixel_dir_box(const rt_camera &cam, float ax, float by, double dlo[3], double dhi[3])
{
    double nmin = 1e300;
    for (int k = 0; k < 3; ++k) {
        dlo[k] = 1e300;
        dhi[k] = -1e300;
    }
    for (int c = 0; c < 4; ++c) {
        const float a = ax + (float)(c & 1), b = by + (float)(c >> 1);
        const V3 d = camera_dir(cam, a, b);
        const double dv[3] = {d.x, d.y, d.z};
        for (int k = 0; k < 3; ++k) {
            dlo[k] = fmin(dlo[k], dv[k]);
            dhi[k] = fmax(dhi[k], dv[k]);
        }
        const double vx = (double)cam.view.x + (double)cam.right.x * a + (double)cam.up.x * b;
        const double vy = (double)cam.view.y + (double)cam.right.y * a + (double)cam.up.y * b;
        const double vz = (double)cam.view.z + (double)cam.right.z * a + (double)cam.up.z * b;
        nmin = fmin(nmin, sqrt(vx * vx + vy * vy + vz * vz));
    }
    const double r2 = (double)cam.right.x * cam.right.x + (double)cam.right.y * cam.right.y +
                      (double)cam.right.z * cam.right.z;
    const double u2 = (double)cam.up.x * cam.up.x + (double)cam.up.y * cam.up.y + (double)cam.up.z * cam.up.z;
    nmin -= sqrt(r2) + sqrt(u2);
    const double bulge = nmin > 1e-3 ? 0.75 * (r2 + u2) / (nmin * nmin) : 2.0; /* 2: the whole direction range */
    const double pad = 1e-5 + bulge;
    for (int k = 0; k < 3; ++k) {
        dlo[k] -= pad;
        dhi[k] += pad;
    }
}

__global__ __launch_bounds__(RT_BLOCK) void k_pixel_lists(RtTriLaunch a, const float *__restrict__ nodes4,
                                                          const uint32_t *__restrict__ q4, uint16_t *__restrict__ codes,
                                                          uint32_t *__restrict__ tile_base)
{
    /* one wave per 8 x 8 pixel tile: neighbouring frusta walk the same nodes */
    __shared__ int s_fstack[kFrustumStack * RT_BLOCK];
    const uint32_t item = blockIdx.x * RT_BLOCK + threadIdx.x, tiles_x = (a.W + 7u) / 8u;
    const uint32_t tile = item >> 6;
    uint32_t x, yl;
    const bool valid = tile_pixel(a, nullptr, tile, item & 63u, tiles_x, x, yl);
    const uint32_t p = yl * a.W + x;
    const float4 *__restrict__ tris = reinterpret_cast<const float4 *>(a.tris);
    int slot[RT_LIST_MAX];
    float key[RT_LIST_MAX];
    uint32_t n = 0;
    bool ok = false;
    if (valid) {
        const uint32_t y = global_row(a, yl);
        /* a = fa - W/2 with fa in [x, x + 1] (the kernel's float subtraction, exact at these
           magnitudes), likewise b */
        const float ax = (float)x - ((float)a.W) / 2.0f, by = (float)y - ((float)a.H) / 2.0f;
        Frustum f;
        pixel_dir_box(a.cam, ax, by, f.dlo, f.dhi);
        pixel_square(f, a.cam, ax, by);
        for (int k = 0; k < 3; ++k) f.o[k] = k == 0 ? a.cam.position.x : k == 1 ? a.cam.position.y : a.cam.position.z;
        frustum_init(f);
        ok = frustum_list(nodes4, q4, tris, f, slot, key, RT_LIST_MAX, n, (lds_int *)(s_fstack + threadIdx.x));
    }
    /* The tile's lists are one block of the list area (one atomic per wave), in lane order, each
       list starting on a 128-B line (a multiple of 8 records of 48 B; the area's base is one too):
       the first records of a list — most camera queries read one to three — then share lines
       (r02's fixed 32-slot layout had that by accident: it read 0.45G fewer lines per frame than
       lists at arbitrary offsets) */
    const uint32_t want = ok ? (n + 7u) & ~7u : 0u;
    const int lane = (int)(threadIdx.x & 63u);
    uint32_t incl = want;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    const uint32_t total = __shfl(incl, 63);
    uint32_t base = 0;
    if (lane == 0 && total) base = atomicAdd(a.list_alloc, total);
    base = __shfl(base, 0);
    /* no room left in the list area: the tile's camera rays take the tree (wave-uniform) */
    if ((uint64_t)base + total > a.list_cap) ok = false;
    const uint32_t n_tiles = tiles_x * ((a.Hl + 7u) / 8u);
    if (lane == 0 && tile < n_tiles) tile_base[tile] = a.list_base + base;
    if (!valid) return;
    const uint32_t rel = incl - want; /* < 64 * RT_LIST_MAX, a multiple of 8 */
    codes[p] = (uint16_t)(!ok ? RT_LIST_NONE : n == 0 ? RT_LIST_EMPTY : ((rel >> 3) << RT_LIST_BITS) | (n - 1u));
    if (!ok || n == 0) return;
    float4 *__restrict__ lst = const_cast<float4 *>(tris) + 3ull * (a.list_base + (size_t)base + rel);
    /* The records in order of their earliest accept t, each one's r1.w carrying the NEXT
       record's bound (+inf on the last): a closest-hit query whose best t is already below
       it has its answer (trav_step_q ends the list there — the accept rule needs t < best_t,
       or t == best_t). */
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t r = 0;
        float next = kInf;
        for (uint32_t j = 0; j < n; ++j) {
            const bool before = key[j] < key[i] || (key[j] == key[i] && j < i);
            r += before ? 1u : 0u;
            if (!before && j != i) next = fminf(next, key[j]);
        }
        const int s = slot[i];
        const float4 e1 = tris[3 * s + 1];
        lst[3 * r] = tris[3 * s];
        lst[3 * r + 1] = make_float4(e1.x, e1.y, e1.z, next);
        lst[3 * r + 2] = tris[3 * s + 2];
    }
}

/* Conservative traversal for k_pixel_lists: every triangle some ray o + t d of the frustum
   could accept under intersects_triangle's tests is listed (`cap` at most: false on
   overflow): its slot, and the earliest t of such an accept.  (Kept in registers and ranked
   afterwards: 4.85 ms per dragon frame, against 5.6 ms for an insertion sort in the list
   itself at 109 instead of 164 VGPRs.) */
__device__ bool frustum_list(const float *__restrict__ nodes4, const uint32_t *__restrict__ q4,
                             const float4 *__restrict__ tris, const Frustum &fr, int *slots, float *keys, uint32_t cap,
                             uint32_t &n, lds_int *stack)
{
    const double *dlo = fr.dlo, *dhi = fr.dhi, *olo = fr.o;
    const double l1 = fr.l1;
    int sp = 0, node = 0;
    n = 0;
    bool ok = true;
    for (;;) {
        const float *f = nodes4 + 32ull * (uint32_t)node;
        for (int k = 0; k < 4 && ok; ++k) {
            const int c = __float_as_int(f[24 + k]);
            if (c == RT_EMPTY_CHILD) continue;
            const double lo[3] = {f[0 + k], f[8 + k], f[16 + k]}, hi[3] = {f[4 + k], f[12 + k], f[20 + k]};
            if (!frustum_slab(fr, lo, hi)) continue;
            if (c >= 0) {
                if (q4) { /* the child's normal box (determinant cull) */
                    const uint32_t wl = q4[(size_t)RT_QNODE_DWORDS * (uint32_t)c + 10];
                    const uint32_t wh = q4[(size_t)RT_QNODE_DWORDS * (uint32_t)c + 11];
                    const double sc = ldexp(1.0, (int)(wl >> 24) - 128);
                    const double nlo[3] = {((int)(wl & 255u) - 128) * sc, ((int)((wl >> 8) & 255u) - 128) * sc,
                                           ((int)((wl >> 16) & 255u) - 128) * sc};
                    const double nhi[3] = {((int)(wh & 255u) - 128) * sc, ((int)((wh >> 8) & 255u) - 128) * sc,
                                           ((int)((wh >> 16) & 255u) - 128) * sc};
                    if (frustum_det(dlo, dhi, nlo, nhi) * 1.02 + 5e-7 * l1 < 1e-4) continue;
                }
                if (sp >= kFrustumStack) {
                    ok = false;
                    break;
                }
                stack[RT_BLOCK * sp++] = c;
                continue;
            }
            const int enc = ~c, first = enc >> 3, cnt = (enc & 7) + 1;
            for (int j = 0; j < cnt; ++j) {
                const int s = first + j;
                const float4 r0 = tris[3 * s], r1 = tris[3 * s + 1], r2 = tris[3 * s + 2];
                double lo[3], hi[3], nmax, tin;
                tri_padded_box(r0, r1, r2, lo, hi, nmax);
                if (!frustum_slab(fr, lo, hi, &tin)) continue;
                const double e1[3] = {r1.x, r1.y, r1.z}, e2[3] = {r2.x, r2.y, r2.z};
                const double nv[3] = {e2[1] * e1[2] - e2[2] * e1[1], e2[2] * e1[0] - e2[0] * e1[2],
                                      e2[0] * e1[1] - e2[1] * e1[0]};
                const double el = (fabs(e1[0]) + fabs(e1[1]) + fabs(e1[2])) * (fabs(e2[0]) + fabs(e2[1]) + fabs(e2[2]));
                if (frustum_det(dlo, dhi, nv, nv) * (1.0 + 1e-6) + 8.0 * 0x1p-24 * l1 * el < 1e-4) continue;
                double tf2 = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double u = fmax(fabs(lo[k] - olo[k]), fabs(hi[k] - olo[k]));
                    tf2 += u * u;
                }
                if (!tri_meets_pixel(fr, r0, r1, r2, sqrt(tf2))) continue;
                if (n >= cap) {
                    ok = false;
                    break;
                }
                /* the earliest t any ray could accept this triangle at: the box entry less the
                   error of the float t (relative ~gamma |e1| |e2| |d| / |det|, |det| >= 1e-4;
                   30x margin), at the farthest t the box allows; kept in the spare r1.w */
                const double le1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
                const double le2 = sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
                const double terr = sqrt(tf2) * (2e-6 * le1 * le2 * l1 / 1e-4 + 1e-6) * l1 + 1e-5;
                /* the float t estimates the exact ray parameter of the triangle's plane, q / (N . d)
                   with q = N . (v0 - o): over the direction box N . d lies in [mlo, mhi], so where
                   that keeps one sign with q, t >= q / mhi (q, mlo > 0) or q / mlo (q, mhi < 0) —
                   for a triangle facing the pixel far later than its box's entry */
                double tpl = -1e300;
                {
                    double mlo = 0.0, mhi = 0.0, q = 0.0;
                    for (int k = 0; k < 3; ++k) {
                        const double a0 = nv[k] * dlo[k], a1 = nv[k] * dhi[k];
                        mlo += fmin(a0, a1);
                        mhi += fmax(a0, a1);
                        q += nv[k] * ((double)(k == 0 ? r0.x : k == 1 ? r0.y : r0.z) - olo[k]);
                    }
                    const double qe = 1e-12 * (fabs(nv[0]) + fabs(nv[1]) + fabs(nv[2])) * (1.0 + sqrt(tf2));
                    if (mlo > 0.0 && q - qe > 0.0) tpl = (q - qe) / (mhi * (1.0 + 1e-12));
                    else if (mhi < 0.0 && q + qe < 0.0) tpl = (q + qe) / (mlo * (1.0 + 1e-12));
                }
                slots[n] = s;
                keys[n] = __double2float_rd(fmax(tin, tpl) - terr);
                ++n;
            }
        }
        if (!ok || sp == 0) break;
        node = stack[RT_BLOCK * --sp];
    }
    return ok;
}

} // namespace

int rt_launch_pixel_lists(const RtTriLaunch &a, const float *nodes4, const uint32_t *q4, uint16_t *codes,
                          uint32_t *tile_base, void *stream)
{
    const uint32_t items = ((a.W + 7u) / 8u) * ((a.Hl + 7u) / 8u) * 64u;
    if (!a.W || !a.Hl) return 0;
    hipError_t e = hipMemsetAsync(a.list_alloc, 0, sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_pixel_lists, dim3((items + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, (hipStream_t)stream,
                       a, nodes4, q4, codes, tile_base);
    return (int)hipGetLastError();
}
