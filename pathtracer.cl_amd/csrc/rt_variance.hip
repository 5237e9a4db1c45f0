/*
 * rt_variance.hip — the variance-guided display filter (gfx950).
 *
 *   k_moments          per pixel: recover the frame's own sample from the accumulation buffer before
 *                      and after it, and keep the running mean of its luminance and of its square
 *   k_variance         per pixel: the variance of the displayed (mean) luminance, from the moments
 *                      where the history is long enough, else from a 7 x 7 feature-weighted window
 *   k_atrous_var, k_atrous_var_lds<S>   one pass of the a-trous filter whose colour term is the
 *                      luminance difference in units of the local standard deviation (Schied et al.
 *                      2017), the variance filtered along with the colour: taps gathered from global
 *                      memory, or (steps 1 and 2) from a tile staged in LDS
 *
 * Nothing in the reference corresponds to these kernels; their arithmetic is pinned in
 * DESIGN.md §4.11 under the model of include/rt_math.h (no contraction, IEEE division and
 * square root, the pinned exponential), so that a float32 restatement reproduces every bit.
 * None touches a render's state, and the accumulation buffer is only read.
 */
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "pathtracer_rt.h"
#include "rt_internal.h"
#include "rt_math.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float lum3(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

/* the sample a progressive frame mixed in: mix(old, s, 1/n) inverted, negative results (rounding) to 0 */
__device__ __forceinline__ float unmix(float prev, float cur, float n)
{
    const float s = prev + (cur - prev) * n;
    return s > 0.0f ? s : 0.0f;
}

/* One lane per pixel; mom_out may be mom_in (each lane reads its pixel before it writes it). */
__global__ __launch_bounds__(256) void k_moments(const float4 *prev, const float4 *cur, float n, float f,
                                                 const float4 *mom_in, float4 *mom_out, uint32_t npx)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npx) return;
    const float4 c = cur[p];
    if (n == 1.0f) { /* the first frame of a view is its own sample; no history is read */
        const float L = lum3(c.x > 0.0f ? c.x : 0.0f, c.y > 0.0f ? c.y : 0.0f, c.z > 0.0f ? c.z : 0.0f);
        mom_out[p] = make_float4(L, L * L, 0.0f, 0.0f);
        return;
    }
    const float4 o = prev[p], m = mom_in[p];
    const float L = lum3(unmix(o.x, c.x, n), unmix(o.y, c.y, n), unmix(o.z, c.z, n));
    mom_out[p] = make_float4(m.x + (L - m.x) * f, m.y + (L * L - m.y) * f, 0.0f, 0.0f);
}

#define RT_VAR_BX 32
#define RT_VAR_BY 8

/* the feature terms of a tap, as atrous_tap's */
__device__ __forceinline__ float feat_arg(float4 pq, float4 nq, float4 pp, float4 np, float isn, float isp, float &ep_isp)
{
    const float dnx = nq.x - np.x, dny = nq.y - np.y, dnz = nq.z - np.z;
    const float en = dnx * dnx + dny * dny + dnz * dnz;
    const float pl = (pq.x - pp.x) * np.x + (pq.y - pp.y) * np.y + (pq.z - pp.z) * np.z;
    const float ep = pl * pl;
    ep_isp = ep * isp;
    return en * isn;
}

/* The 49 taps of the spatial estimate are gathered from global memory (only pixels with a short
   history take that path: the frames after a disocclusion or a reshape). */
__global__ __launch_bounds__(RT_VAR_BX *RT_VAR_BY) void k_variance(const float4 *__restrict__ disp,
                                                                    const float4 *__restrict__ mom,
                                                                    const float *__restrict__ len,
                                                                    const float4 *__restrict__ feat,
                                                                    float *__restrict__ out, uint32_t W, uint32_t H,
                                                                    float isn, float isp, float min_len)
{
    const int x = (int)(blockIdx.x * RT_VAR_BX + threadIdx.x);
    const int y = (int)(blockIdx.y * RT_VAR_BY + threadIdx.y);
    if (x >= (int)W || y >= (int)H) return;
    const float4 *__restrict__ pos = feat;
    const float4 *__restrict__ nrm = feat + (size_t)W * H;
    const size_t p = (size_t)y * W + x;
    const float l = len[p];
    if (l >= min_len) {
        const float4 m = mom[p];
        const float d = m.y - m.x * m.x;
        out[p] = (d > 0.0f ? d : 0.0f) / (l - 1.0f);
        return;
    }
    const float4 pp = pos[p], np = nrm[p];
    float a1 = 0.0f, a2 = 0.0f, ws = 0.0f;
    for (int dy = -3; dy <= 3; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)H) continue;
        for (int dx = -3; dx <= 3; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)W) continue;
            const size_t q = (size_t)qy * W + qx;
            float ep_isp;
            const float en_isn = feat_arg(pos[q], nrm[q], pp, np, isn, isp, ep_isp);
            const float w = rt_expf(-(en_isn + ep_isp));
            const float4 cq = disp[q];
            const float Lq = lum3(cq.x, cq.y, cq.z);
            a1 += Lq * w;
            a2 += (Lq * Lq) * w;
            ws += w;
        }
    }
    const float m1 = a1 / ws, m2 = a2 / ws;
    const float d = m2 - m1 * m1;
    out[p] = (d > 0.0f ? d : 0.0f) * (min_len / (l > 1.0f ? l : 1.0f));
}

/* ---- the filter.  Tap order as DESIGN.md §4.9: dy outer, dx inner, a tap outside the frame
   skipped; how the four streams of a tap (colour, P, N, variance) reach the lane is the kernels'. */
struct VarAcc {
    float x, y, z, wsum, v;
};

/* one tap: w = h exp(-((el + en isn) + ep isp)), acc += c_q w, vacc += v_q w^2 */
__device__ __forceinline__ void var_tap(VarAcc &acc, float h, float4 cq, float4 pq, float4 nq, float vq, float lp,
                                        float4 pp, float4 np, float il, float isn, float isp)
{
    const float el = fabsf(lum3(cq.x, cq.y, cq.z) - lp) * il;
    float ep_isp;
    const float en_isn = feat_arg(pq, nq, pp, np, isn, isp, ep_isp);
    const float w = h * rt_expf(-((el + en_isn) + ep_isp));
    acc.x += cq.x * w;
    acc.y += cq.y * w;
    acc.z += cq.z * w;
    acc.wsum += w;
    acc.v += vq * (w * w);
}

__device__ __forceinline__ float var_h(int dx, int dy)
{
    const float k[3] = {0.375f, 0.25f, 0.0625f};
    return k[dx < 0 ? -dx : dx] * k[dy < 0 ? -dy : dy];
}

__device__ __forceinline__ float gauss_k(int dx, int dy)
{
    const float kg[3] = {0.25f, 0.125f, 0.0625f};
    return kg[(dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)];
}

/* the luminance term's inverse tolerance from the prefiltered variance g (lum_on == 0: the term is off) */
__device__ __forceinline__ float inv_lum(float g, float sigma_lum, int lum_on)
{
    return lum_on ? 1.0f / (sigma_lum * rt_sqrtf(g) + 1e-8f) : 0.0f;
}

__device__ __forceinline__ void var_store(float4 *out, float *out_var, size_t p, const VarAcc &acc, float alpha)
{
    out[p] = make_float4(acc.x / acc.wsum, acc.y / acc.wsum, acc.z / acc.wsum, alpha);
    if (out_var) out_var[p] = acc.v / (acc.wsum * acc.wsum);
}

/* The gather form (steps 4 and up), as k_atrous. */
__global__ __launch_bounds__(RT_VAR_BX *RT_VAR_BY) void k_atrous_var(const float4 *__restrict__ col,
                                                                      const float *__restrict__ var,
                                                                      const float4 *__restrict__ feat,
                                                                      float4 *__restrict__ out, float *__restrict__ out_var,
                                                                      uint32_t W, uint32_t H, int step, float sigma_lum,
                                                                      int lum_on, float isn, float isp)
{
    const int x = (int)(blockIdx.x * RT_VAR_BX + threadIdx.x);
    const int y = (int)(blockIdx.y * RT_VAR_BY + threadIdx.y);
    if (x >= (int)W || y >= (int)H) return;
    const float4 *__restrict__ pos = feat;
    const float4 *__restrict__ nrm = feat + (size_t)W * H;
    const size_t p = (size_t)y * W + x;
    float ga = 0.0f, gs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= (int)W || qy < 0 || qy >= (int)H) continue;
            const float kg = gauss_k(dx, dy);
            ga += var[(size_t)qy * W + qx] * kg;
            gs += kg;
        }
    }
    const float il = inv_lum(ga / gs, sigma_lum, lum_on);
    const float4 cp = col[p], pp = pos[p], np = nrm[p];
    const float lp = lum3(cp.x, cp.y, cp.z);
    VarAcc acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + step * dy;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= (int)W || qy < 0 || qy >= (int)H) continue;
            const size_t q = (size_t)qy * W + qx;
            var_tap(acc, var_h(dx, dy), col[q], pos[q], nrm[q], var[q], lp, pp, np, il, isn, isp);
        }
    }
    var_store(out, out_var, p, acc, cp.w);
}

/* The staged form (steps S = 1 and 2): the tile and its halo of 2 S pixels, (32 + 4 S) x (8 + 4 S)
   cells of the four streams (52 B a cell: 22,464 B / 33,280 B), loaded once into LDS.  The streams
   are planes of their own: a lane row reads consecutive 16-B cells of a float4 plane
   (conflict-free ds_read_b128) and consecutive dwords of the variance plane (32 lanes on 32 banks:
   conflict-free ds_read_b32); interleaved 52-B cells would leave the 16-B reads unaligned.  The
   unit-distance prefilter stays inside the halo (1 <= 2 S).  Cells outside the frame are neither
   written nor read. */
template <int S>
__global__ __launch_bounds__(RT_VAR_BX *RT_VAR_BY) void k_atrous_var_lds(const float4 *__restrict__ col,
                                                                          const float *__restrict__ var,
                                                                          const float4 *__restrict__ feat,
                                                                          float4 *__restrict__ out,
                                                                          float *__restrict__ out_var, uint32_t W, uint32_t H,
                                                                          float sigma_lum, int lum_on, float isn, float isp)
{
    constexpr int TW = RT_VAR_BX + 4 * S, TH = RT_VAR_BY + 4 * S;
    __shared__ float4 s_c[TW * TH], s_p[TW * TH], s_n[TW * TH];
    __shared__ float s_v[TW * TH];
    const float4 *__restrict__ pos = feat;
    const float4 *__restrict__ nrm = feat + (size_t)W * H;
    const int x0 = (int)(blockIdx.x * RT_VAR_BX) - 2 * S, y0 = (int)(blockIdx.y * RT_VAR_BY) - 2 * S;
    const int tid = (int)(threadIdx.y * RT_VAR_BX + threadIdx.x);
    for (int i = tid; i < TW * TH; i += RT_VAR_BX * RT_VAR_BY) {
        const int gx = x0 + i % TW, gy = y0 + i / TW;
        if (gx >= 0 && gx < (int)W && gy >= 0 && gy < (int)H) {
            const size_t q = (size_t)gy * W + gx;
            s_c[i] = col[q];
            s_p[i] = pos[q];
            s_n[i] = nrm[q];
            s_v[i] = var[q];
        }
    }
    __syncthreads();
    const int x = (int)(blockIdx.x * RT_VAR_BX + threadIdx.x);
    const int y = (int)(blockIdx.y * RT_VAR_BY + threadIdx.y);
    if (x >= (int)W || y >= (int)H) return;
    const int lp = ((int)threadIdx.y + 2 * S) * TW + (int)threadIdx.x + 2 * S;
    float ga = 0.0f, gs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= (int)W || qy < 0 || qy >= (int)H) continue;
            const float kg = gauss_k(dx, dy);
            ga += s_v[lp + dy * TW + dx] * kg;
            gs += kg;
        }
    }
    const float il = inv_lum(ga / gs, sigma_lum, lum_on);
    const float4 cp = s_c[lp], pp = s_p[lp], np = s_n[lp];
    const float lpl = lum3(cp.x, cp.y, cp.z);
    VarAcc acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + S * dy;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + S * dx;
            if (qx < 0 || qx >= (int)W || qy < 0 || qy >= (int)H) continue;
            const int q = lp + S * dy * TW + S * dx;
            var_tap(acc, var_h(dx, dy), s_c[q], s_p[q], s_n[q], s_v[q], lpl, pp, np, il, isn, isp);
        }
    }
    var_store(out, out_var, (size_t)y * W + x, acc, cp.w);
}

} // namespace

int rt_launch_moments(const float *prev_rgba, const float *cur_rgba, float n_cur, const float *mom_in, float *mom_out,
                      uint32_t W, uint32_t H, void *stream)
{
    const uint32_t npx = W * H; /* < 2^28 (the host's frame check) */
    hipLaunchKernelGGL(k_moments, dim3((npx + 255u) / 256u), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(prev_rgba), reinterpret_cast<const float4 *>(cur_rgba), n_cur,
                       1.0f / n_cur, reinterpret_cast<const float4 *>(mom_in), reinterpret_cast<float4 *>(mom_out), npx);
    return (int)hipGetLastError();
}

int rt_launch_variance(const float *disp_rgba, const float *mom_rgba, const float *len, const float *feat, float *out_var,
                       uint32_t W, uint32_t H, float isn, float isp, float min_len, void *stream)
{
    const dim3 grid((W + RT_VAR_BX - 1) / RT_VAR_BX, (H + RT_VAR_BY - 1) / RT_VAR_BY);
    hipLaunchKernelGGL(k_variance, grid, dim3(RT_VAR_BX, RT_VAR_BY), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(disp_rgba), reinterpret_cast<const float4 *>(mom_rgba), len,
                       reinterpret_cast<const float4 *>(feat), out_var, W, H, isn, isp, min_len);
    return (int)hipGetLastError();
}

int rt_launch_atrous_var(const float *col, const float *var, const float *feat, float *out, float *out_var, uint32_t W,
                         uint32_t H, uint32_t step, float sigma_lum, int lum_on, float isn, float isp, void *stream)
{
    const dim3 grid((W + RT_VAR_BX - 1) / RT_VAR_BX, (H + RT_VAR_BY - 1) / RT_VAR_BY);
    const dim3 block(RT_VAR_BX, RT_VAR_BY);
    const float4 *c4 = reinterpret_cast<const float4 *>(col), *f4 = reinterpret_cast<const float4 *>(feat);
    float4 *o4 = reinterpret_cast<float4 *>(out);
    hipStream_t st = (hipStream_t)stream;
    /* steps 1 and 2 from LDS, the larger ones gathered, as rt_launch_atrous; RTMI_ATROUS_LDS (A/B
       knob, no result bit depends on it): the largest step staged, 0 = none */
    const char *knob = getenv("RTMI_ATROUS_LDS");
    const uint32_t lds_max = knob ? (uint32_t)atoi(knob) : 2u;
    if (step <= 2 && step <= lds_max) {
        if (step == 1)
            hipLaunchKernelGGL(k_atrous_var_lds<1>, grid, block, 0, st, c4, var, f4, o4, out_var, W, H, sigma_lum, lum_on,
                               isn, isp);
        else
            hipLaunchKernelGGL(k_atrous_var_lds<2>, grid, block, 0, st, c4, var, f4, o4, out_var, W, H, sigma_lum, lum_on,
                               isn, isp);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(k_atrous_var, grid, block, 0, st, c4, var, f4, o4, out_var, W, H, (int)step, sigma_lum, lum_on, isn,
                       isp);
    return (int)hipGetLastError();
}
