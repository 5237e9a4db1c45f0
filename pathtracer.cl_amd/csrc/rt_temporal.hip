/*
 * rt_temporal.hip — temporal reprojection of the displayed frame across camera moves (gfx950).
 *
 *   k_reproject        per pixel of the new view: project its first-hit position into the previous
 *                      view, gather the four bilinear taps of the previous displayed frame that lie
 *                      on the same surface, and carry their colour and history length over
 *   k_temporal_merge   per pixel: blend the carried history with the accumulation buffer by their
 *                      frame counts — the accumulation's one count for the frame, or (PER_PIXEL) a
 *                      plane of them
 *   k_history_trust    per pixel: test the carried history against the accumulation buffer over a
 *                      7 x 7 feature-weighted window staged in LDS, and shorten the history length
 *                      where the two disagree by more than the window's noise explains; the
 *                      accumulation's frame count as in the merge
 *
 * Nothing in the reference corresponds to these kernels; their arithmetic is pinned in
 * DESIGN.md §4.10 and §4.14 under the model of include/rt_math.h (no contraction, IEEE division,
 * the pinned exponential), so that a float32 restatement reproduces every bit.  None touches a
 * render's state, and none writes any of its inputs (the merge may write its history operands in
 * place).
 */
#include <hip/hip_runtime.h>

#include "rt_display_util.h"

#pragma clang fp contract(off)

namespace {

struct ReprojArgs {
    const float4 *prev_col;
    const float *prev_len;
    const float4 *prev_feat;
    const float4 *cur_feat;
    float4 *out_col;
    float *out_len;
    /* the previous camera's position and the cofactor columns of (view, right, up): cs = right x up,
       ca = up x view, cb = view x right; det = view . cs (rt_launch_reproject) */
    float px, py, pz;
    float csx, csy, csz, cax, cay, caz, cbx, cby, cbz, det;
    uint32_t W, H;
    float plane_tol, normal_min, max_history;
};

/* One lane per pixel of the block's RT_TILE_BX x RT_TILE_BY tile.  The taps are gathered straight
   from global memory: for the small camera moves this stage exists for, neighbouring lanes project
   onto neighbouring pixels of the previous frame, so a wave's taps share cache lines (vector L1 /
   L2). */
__global__ __launch_bounds__(RT_TILE_BX *RT_TILE_BY) void k_reproject(ReprojArgs a)
{
    const int x = (int)(blockIdx.x * RT_TILE_BX + threadIdx.x);
    const int y = (int)(blockIdx.y * RT_TILE_BY + threadIdx.y);
    const int W = (int)a.W, H = (int)a.H;
    if (x >= W || y >= H) return;
    const size_t npx = (size_t)a.W * a.H, p = (size_t)y * a.W + x;
    const float4 pp = a.cur_feat[p], np = a.cur_feat[npx + p];
    const int idp = __float_as_int(np.w);
    float ox = 0.0f, oy = 0.0f, oz = 0.0f, ol = 0.0f;
    if (idp != RT_FEAT_NONE && a.det != 0.0f) {
        /* P - position = s (view + a right + b up): Cramer, s = ns / det, a = na / ns, b = nb / ns */
        const float dx = pp.x - a.px, dy = pp.y - a.py, dz = pp.z - a.pz;
        const float ns = (dx * a.csx + dy * a.csy) + dz * a.csz;
        const float na = (dx * a.cax + dy * a.cay) + dz * a.caz;
        const float nb = (dx * a.cbx + dy * a.cby) + dz * a.cbz;
        const float s = ns / a.det;
        if (s > 0.0f) { /* in front of the previous camera (false for a NaN) */
            const float fx = ((na / ns) + ((float)a.W) / 2.0f) - 0.5f;
            const float fy = ((nb / ns) + ((float)a.H) / 2.0f) - 0.5f;
            /* in float, before any conversion: false for a NaN or an infinity, and every tap of a
               coordinate outside (-1, W) x (-1, H) is outside the frame */
            if (fx > -1.0f && fx < (float)a.W && fy > -1.0f && fy < (float)a.H) {
                const float x0f = floorf(fx), y0f = floorf(fy);
                const int x0 = (int)x0f, y0 = (int)y0f; /* in [-1, W-1] x [-1, H-1] */
                const float wx1 = fx - x0f, wy1 = fy - y0f;
                const float wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
                const float tol = a.plane_tol * pp.w;
                float ax = 0.0f, ay = 0.0f, az = 0.0f, al = 0.0f, wsum = 0.0f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int qx = x0 + i, qy = y0 + j;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        const size_t q = (size_t)qy * a.W + (size_t)qx;
                        const float m = a.prev_len[q];
                        if (!(m > 0.0f)) continue;
                        const float4 nq = a.prev_feat[npx + q];
                        const int idq = __float_as_int(nq.w);
                        if (idq == RT_FEAT_NONE) continue;
                        if (!same_surface_class(idp, idq)) continue;
                        const float4 pq = a.prev_feat[q];
                        const float pl = ((pq.x - pp.x) * np.x + (pq.y - pp.y) * np.y) + (pq.z - pp.z) * np.z;
                        if (!(fabsf(pl) <= tol)) continue;
                        const float nn = (nq.x * np.x + nq.y * np.y) + nq.z * np.z;
                        if (!(nn >= a.normal_min)) continue;
                        const float w = (i ? wx1 : wx0) * (j ? wy1 : wy0);
                        const float4 cq = a.prev_col[q];
                        ax = ax + w * cq.x;
                        ay = ay + w * cq.y;
                        az = az + w * cq.z;
                        al = al + w * m;
                        wsum = wsum + w;
                    }
                }
                if (wsum > 0.0f) {
                    ox = ax / wsum;
                    oy = ay / wsum;
                    oz = az / wsum;
                    const float l = al / wsum;
                    ol = l < a.max_history ? l : a.max_history;
                }
            }
        }
    }
    a.out_col[p] = make_float4(ox, oy, oz, 0.0f);
    a.out_len[p] = ol;
}

/* the accumulation buffer's frame count at a pixel of a plane of them: 1 under 1 (a NaN and the 0 of a
   tile stopped before its first fold among them) */
__device__ __forceinline__ float frames_at(const float *cur_len, size_t p)
{
    const float v = cur_len[p];
    return v >= 1.0f ? v : 1.0f;
}

/* out = h + (c - h) (n / (n + m)) where the history is m > 0 frames long, c's bits elsewhere; h, m
   and the outputs may be the same buffers (each lane reads its pixel before it writes it).  PER_PIXEL:
   n is the pixel's own of cur_len (apart from the outputs), else n_all. */
template <bool PER_PIXEL>
__global__ __launch_bounds__(kPixelBlock) void k_temporal_merge(const float4 *hist, const float *hist_len, const float4 *cur,
                                                        float n_all, const float *cur_len, float max_history, float4 *out,
                                                        float *out_len, uint32_t npx)
{
    const uint32_t p = blockIdx.x * kPixelBlock + threadIdx.x;
    if (p >= npx) return;
    const float4 c = cur[p];
    const float m = hist_len[p];
    const float n = PER_PIXEL ? frames_at(cur_len, p) : n_all;
    float4 o = c;
    float l = n;
    if (m > 0.0f) {
        const float4 h = hist[p];
        l = n + m;
        const float f = n / l;
        o.x = h.x + (c.x - h.x) * f;
        o.y = h.y + (c.y - h.y) * f;
        o.z = h.z + (c.z - h.z) * f;
    }
    out[p] = o;
    out_len[p] = l < max_history ? l : max_history;
}

struct TrustArgs {
    const float4 *hist;
    const float4 *cur;
    const float *hist_len;
    const float4 *feat;
    const float *cur_len; /* PER_PIXEL: the accumulation's frame counts; else n */
    float *out_len;
    uint32_t W, H;
    float n, k2, isn, isp;
};

constexpr int TRUST_R = 3; /* the 7 x 7 window */
constexpr int TRUST_TW = RT_TILE_BX + 2 * TRUST_R, TRUST_TH = RT_TILE_BY + 2 * TRUST_R, TRUST_CELLS = TRUST_TW * TRUST_TH;

/* One lane per pixel of the block's RT_TILE_BX x RT_TILE_BY tile.  The tile and
   its halo of 3 pixels — 38 x 14 cells — are staged in LDS once: per cell the luminance of the
   accumulation buffer and of the history (computed here, so the 49 taps of a pixel read two dwords
   where the frame holds two float4), P and N with the surface id.  Planes of their own, as the
   a-trous pass keeps them (rt_filter.hip): a lane row reads consecutive 16-B cells or consecutive
   dwords.  40 B a cell, 21,280 B a block.  A cell that cannot count as a tap — outside the frame,
   without history, or on no surface — is staged as the id RT_FEAT_NONE alone: none of its streams
   is loaded or read.  (A centre pixel that has a history length and a surface is itself such a
   cell that counts, so its own P, N and id come from the tile.)  The taps are summed in the
   definition's order, dy outer, dx inner, whatever the staging.  out_len apart from every input:
   a neighbouring block reads hist_len for its halo (the host keeps an in-place call apart).
   PER_PIXEL: the accumulation's frame count is the centre pixel's own of cur_len — one dword more a
   lane, the staging as it is: the taps of a window that reaches into tiles of other counts are
   weighed as if they had the centre's. */
template <bool PER_PIXEL> __global__ __launch_bounds__(RT_TILE_BX *RT_TILE_BY) void k_history_trust(TrustArgs a)
{
    __shared__ float4 s_p[TRUST_CELLS], s_n[TRUST_CELLS];
    __shared__ float s_lc[TRUST_CELLS], s_lh[TRUST_CELLS];
    const int W = (int)a.W, H = (int)a.H;
    const size_t npx = (size_t)a.W * a.H;
    const int x0 = (int)(blockIdx.x * RT_TILE_BX) - TRUST_R, y0 = (int)(blockIdx.y * RT_TILE_BY) - TRUST_R;
    const int tid = (int)(threadIdx.y * RT_TILE_BX + threadIdx.x);
    for (int i = tid; i < TRUST_CELLS; i += RT_TILE_BX * RT_TILE_BY) {
        const int gx = x0 + i % TRUST_TW, gy = y0 + i / TRUST_TW;
        float4 nq = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(RT_FEAT_NONE));
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t q = (size_t)gy * a.W + gx;
            if (a.hist_len[q] > 0.0f) {
                nq = a.feat[npx + q];
                if (__float_as_int(nq.w) != RT_FEAT_NONE) {
                    s_p[i] = a.feat[q];
                    s_lc[i] = lum3(a.cur[q]);
                    s_lh[i] = lum3(a.hist[q]);
                }
            }
        }
        s_n[i] = nq;
    }
    __syncthreads();
    const int x = (int)(blockIdx.x * RT_TILE_BX + threadIdx.x);
    const int y = (int)(blockIdx.y * RT_TILE_BY + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * a.W + x;
    const float m = a.hist_len[p];
    const float n = PER_PIXEL ? frames_at(a.cur_len, p) : a.n;
    if (!(m > 0.0f)) { /* no history (false for a NaN too) */
        a.out_len[p] = 0.0f;
        return;
    }
    const int c0 = ((int)threadIdx.y + TRUST_R) * TRUST_TW + (int)threadIdx.x + TRUST_R;
    const float4 np = s_n[c0];
    const int idp = __float_as_int(np.w);
    if (idp == RT_FEAT_NONE) { /* no surface to compare on */
        a.out_len[p] = m;
        return;
    }
    const float4 pp = s_p[c0];
    float ws = 0.0f, w2 = 0.0f, ac = 0.0f, ac2 = 0.0f, ah = 0.0f, ah2 = 0.0f;
    for (int dy = -TRUST_R; dy <= TRUST_R; ++dy) {
#pragma unroll
        for (int dx = -TRUST_R; dx <= TRUST_R; ++dx) {
            const int q = c0 + dy * TRUST_TW + dx;
            const float4 nq = s_n[q];
            const int idq = __float_as_int(nq.w);
            if (idq == RT_FEAT_NONE) continue;
            if (!same_surface_class(idp, idq)) continue;
            /* all of a tap's loads before its weight (rt_expf branches) */
            const float4 pq = s_p[q];
            const float Lc = s_lc[q], Lh = s_lh[q];
            float ep_isp;
            const float en_isn = feat_arg(pq, nq, pp, np, a.isn, a.isp, ep_isp);
            const float w = rt_expf(-(en_isn + ep_isp));
            ws += w;
            w2 += w * w;
            ac += Lc * w;
            ac2 += (Lc * Lc) * w;
            ah += Lh * w;
            ah2 += (Lh * Lh) * w;
        }
    }
    const float mc = ac / ws, mh = ah / ws;
    const float dc = ac2 / ws - mc * mc, dh = ah2 / ws - mh * mh;
    const float vc = dc > 0.0f ? dc : 0.0f, vh = dh > 0.0f ? dh : 0.0f;
    const float ne = w2 / (ws * ws);
    float o = m;
    if (!(ne > 0.5f)) { /* two effective taps at least: there is something to judge by */
        const float vs = vh * ((m > 1.0f ? m : 1.0f) / n);
        const float v = vc > vs ? vc : vs;
        const float vd = (v * ne) * (1.0f + n / m) + 1e-12f;
        const float d = mc - mh;
        const float z2 = (d * d) / vd;
        if (z2 > a.k2) o = m * (a.k2 / z2);
    }
    a.out_len[p] = o;
}

} // namespace

int rt_launch_reproject(const float *prev_rgba, const float *prev_len, const float *prev_feat, const rt_camera &cam,
                        const float *cur_feat, float *out_rgba, float *out_len, uint32_t W, uint32_t H, float plane_tol,
                        float normal_min, float max_history, void *stream)
{
    ReprojArgs a;
    a.prev_col = reinterpret_cast<const float4 *>(prev_rgba);
    a.prev_len = prev_len;
    a.prev_feat = reinterpret_cast<const float4 *>(prev_feat);
    a.cur_feat = reinterpret_cast<const float4 *>(cur_feat);
    a.out_col = reinterpret_cast<float4 *>(out_rgba);
    a.out_len = out_len;
    const rt_float4 &v = cam.view, &r = cam.right, &u = cam.up;
    a.px = cam.position.x;
    a.py = cam.position.y;
    a.pz = cam.position.z;
    /* cross(a, b) = (ay bz - az by, az bx - ax bz, ax by - ay bx), each product and difference rounded */
    a.csx = r.y * u.z - r.z * u.y;
    a.csy = r.z * u.x - r.x * u.z;
    a.csz = r.x * u.y - r.y * u.x;
    a.cax = u.y * v.z - u.z * v.y;
    a.cay = u.z * v.x - u.x * v.z;
    a.caz = u.x * v.y - u.y * v.x;
    a.cbx = v.y * r.z - v.z * r.y;
    a.cby = v.z * r.x - v.x * r.z;
    a.cbz = v.x * r.y - v.y * r.x;
    a.det = (v.x * a.csx + v.y * a.csy) + v.z * a.csz;
    a.W = W;
    a.H = H;
    a.plane_tol = plane_tol;
    a.normal_min = normal_min;
    a.max_history = max_history;
    hipLaunchKernelGGL(k_reproject, tile_grid(W, H), tile_block(), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int rt_launch_temporal_merge(const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                             const float *cur_len, float max_history, float *out_rgba, float *out_len, uint32_t W, uint32_t H,
                             void *stream)
{
    const uint32_t npx = W * H; /* < 2^28 (the host's frame check) */
    const auto kernel = cur_len ? k_temporal_merge<true> : k_temporal_merge<false>;
    hipLaunchKernelGGL(kernel, pixel_grid(npx), dim3(kPixelBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(hist_rgba), hist_len, reinterpret_cast<const float4 *>(cur_rgba),
                       n_cur, cur_len, max_history, reinterpret_cast<float4 *>(out_rgba), out_len, npx);
    return (int)hipGetLastError();
}

int rt_launch_history_trust(const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                            const float *cur_len, const float *feat, float *out_len, uint32_t W, uint32_t H, float k2,
                            float isn, float isp, void *stream)
{
    TrustArgs a;
    a.hist = reinterpret_cast<const float4 *>(hist_rgba);
    a.cur = reinterpret_cast<const float4 *>(cur_rgba);
    a.hist_len = hist_len;
    a.feat = reinterpret_cast<const float4 *>(feat);
    a.cur_len = cur_len;
    a.out_len = out_len;
    a.W = W;
    a.H = H;
    a.n = n_cur;
    a.k2 = k2;
    a.isn = isn;
    a.isp = isp;
    const auto kernel = cur_len ? k_history_trust<true> : k_history_trust<false>;
    hipLaunchKernelGGL(kernel, tile_grid(W, H), tile_block(), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
