/*
 * rt_filter.hip — the display filters: luminance moments, variance, and the a-trous pass (gfx950).
 *
 *   k_moments          per pixel: recover the frame's own sample from the accumulation buffer before
 *                      and after it, and keep the running mean of its luminance and of its square
 *   k_moments_tiles    the same on the pixels of the live tiles of a stop plane, with the per-pixel
 *                      history lengths; a stopped tile's pixels keep their moments
 *   k_fold_tiles       a wave per 8x8 tile: the progressive mix of a frame's own sample into the
 *                      accumulation buffer with a weight per tile, from a count plane, and the moments
 *                      and history lengths that go with it
 *   k_variance         per pixel: the variance of the displayed (mean) luminance, from the moments
 *                      where the history is long enough, else from a 7 x 7 feature-weighted window
 *   k_atrous, k_atrous_lds<S>           one pass of the a-trous wavelet filter (Dammertz et al. 2010)
 *                      guided by the first-hit features, its colour term the colour distance
 *   k_atrous_var, k_atrous_var_lds<S>   the same pass with the luminance difference in units of the
 *                      local standard deviation as colour term (Schied et al. 2017), the variance
 *                      filtered along with the colour
 *
 * The six a-trous kernels are one pass (atrous_pass) over its form — taps gathered from global
 * memory, or (steps 1 and 2) from a tile staged in LDS — and its colour term.
 *
 * Nothing in the reference corresponds to these kernels; their arithmetic is pinned in
 * DESIGN.md §4.9 and §4.11 under the model of include/rt_math.h (no contraction, IEEE division and
 * square root, the pinned exponential), so that a float32 restatement reproduces every bit.
 * None touches a render's state, and the accumulation buffer is only read — but for k_fold_tiles,
 * the one display-side kernel that writes it.
 */
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "rt_display_util.h"

#pragma clang fp contract(off)

namespace {

/* the sample a progressive frame mixed in: mix(old, s, 1/n) inverted, negative results (rounding) to 0 */
__device__ __forceinline__ float unmix(float prev, float cur, float n)
{
    const float s = prev + (cur - prev) * n;
    return s > 0.0f ? s : 0.0f;
}

/* a pixel's moments after the first frame of a view, which is its own sample: no history */
__device__ __forceinline__ float4 moments_first(float4 c)
{
    const float L = lum3(c.x > 0.0f ? c.x : 0.0f, c.y > 0.0f ? c.y : 0.0f, c.z > 0.0f ? c.z : 0.0f);
    return make_float4(L, L * L, 0.0f, 0.0f);
}

/* ... and after frame n > 1 (f = 1 / n), which took the pixel from o to c: m with the sample's luminance mixed in */
__device__ __forceinline__ float4 moments_next(float4 o, float4 c, float4 m, float n, float f)
{
    const float L = lum3(unmix(o.x, c.x, n), unmix(o.y, c.y, n), unmix(o.z, c.z, n));
    return make_float4(m.x + (L - m.x) * f, m.y + (L * L - m.y) * f, 0.0f, 0.0f);
}

/* pixel p's moments after a frame; mom_out may be mom_in (the pixel is read before it is written) */
__device__ __forceinline__ void moments_pixel(const float4 *prev, const float4 *cur, float n, float f, const float4 *mom_in,
                                              float4 *mom_out, uint32_t p)
{
    const float4 c = cur[p];
    if (n == 1.0f) { /* the first frame of a view is its own sample; no history is read */
        mom_out[p] = moments_first(c);
        return;
    }
    mom_out[p] = moments_next(prev[p], c, mom_in[p], n, f);
}

/* One lane per pixel. */
__global__ __launch_bounds__(kPixelBlock) void k_moments(const float4 *prev, const float4 *cur, float n, float f,
                                                 const float4 *mom_in, float4 *mom_out, uint32_t npx)
{
    const uint32_t p = blockIdx.x * kPixelBlock + threadIdx.x;
    if (p >= npx) return;
    moments_pixel(prev, cur, n, f, mom_in, mom_out, p);
}

/* The same under a stop plane: a stopped tile's pixels were not traced, so cur ==
   prev there and the recovered "sample" would be the pixel's own mean; they keep their moments, and
   their history length is the frame count their tile stopped at. */
__global__ __launch_bounds__(kPixelBlock) void k_moments_tiles(const float4 *prev, const float4 *cur, float n, float f,
                                                               const float4 *mom_in, float4 *mom_out,
                                                               const uint32_t *__restrict__ stop, float *__restrict__ len_out,
                                                               uint32_t W, uint32_t tw, uint32_t npx)
{
    const uint32_t p = blockIdx.x * kPixelBlock + threadIdx.x;
    if (p >= npx) return;
    const uint32_t y = p / W, x = p - y * W;
    const uint32_t s = stop[(y >> 3) * tw + (x >> 3)];
    if (s) {
        if (mom_in && mom_out != mom_in) mom_out[p] = mom_in[p];
        len_out[p] = (float)s;
        return;
    }
    moments_pixel(prev, cur, n, f, mom_in, mom_out, p);
    len_out[p] = n;
}

/* The progressive mix of a frame's own sample into the accumulation buffer, a weight per 8x8 tile
   (DESIGN.md §4.19), with the moments and the history lengths of the frame it makes.  One wave per
   tile, lane j = (y & 7) 8 + (x & 7), kHistWaves horizontally adjacent tiles a block as in
   k_noise_hist: a wave's pixel rows are 128-byte segments.  The tile's count is read once by the whole
   wave (one address) and written by one lane, whose store waits for that load: no other wave touches
   the word, so the update in place is safe.  The mix is write_pixel's (rt_kernel_util.h): subtract,
   multiply, add, at p == 1 too.  passes null: every tile is folded; mom_in and mom_out both or neither;
   len_out may be null. */
__global__ __launch_bounds__(kHistBlock) void k_fold_tiles(const float4 *__restrict__ sample, float4 *acc, uint32_t *count,
                                                           const uint32_t *__restrict__ passes, uint32_t pass,
                                                           const float4 *mom_in, float4 *mom_out, float *__restrict__ len_out,
                                                           uint32_t W, uint32_t H, uint32_t tw, uint32_t gw)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ty = blockIdx.x / gw, tx = (blockIdx.x - ty * gw) * kHistWaves + wave;
    if (tx >= tw) return; /* (the whole wave) */
    const uint32_t t = ty * tw + tx;
    const uint32_t c = count[t];
    const bool folded = !passes || passes[t] > pass;
    const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
    const bool inside = x < W && y < H;
    const uint32_t p = y * W + x; /* < 2^28 where inside */
    if (!folded) {
        if (inside) {
            if (mom_out && mom_out != mom_in) mom_out[p] = mom_in[p];
            if (len_out) len_out[p] = (float)c;
        }
        return;
    }
    const uint32_t pc = c == 0xffffffffu ? c : c + 1u;
    const float n = (float)pc, w = 1.0f / n;
    if (inside) {
        const float4 s = sample[p], o = acc[p];
        float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (mom_out && n != 1.0f) m = mom_in[p]; /* (uniform; in flight with the other two) */
        const float4 v = make_float4(o.x + (s.x - o.x) * w, o.y + (s.y - o.y) * w, o.z + (s.z - o.z) * w, o.w + (s.w - o.w) * w);
        acc[p] = v;
        if (mom_out) mom_out[p] = n == 1.0f ? moments_first(v) : moments_next(o, v, m, n, w);
        if (len_out) len_out[p] = n;
    }
    if (lane == 0u) count[t] = pc;
}

/* The 49 taps of the spatial estimate are gathered from global memory (only pixels with a short
   history take that path: the frames after a disocclusion or a reshape). */
__global__ __launch_bounds__(RT_TILE_BX *RT_TILE_BY) void k_variance(const float4 *__restrict__ disp,
                                                                      const float4 *__restrict__ mom,
                                                                      const float *__restrict__ len,
                                                                      const float4 *__restrict__ feat,
                                                                      float *__restrict__ out, uint32_t W, uint32_t H,
                                                                      float isn, float isp, float min_len)
{
    const int x = (int)(blockIdx.x * RT_TILE_BX + threadIdx.x);
    const int y = (int)(blockIdx.y * RT_TILE_BY + threadIdx.y);
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

/* ---- the a-trous pass.  A colour term supplies the colour argument of a tap's weight from the
   tap's colour, after centre() has seen the centre pixel's colour and g, the 3 x 3 prefilter of the
   variance plane there; has_var: the pass reads that plane and filters it along. */

/* rt_denoise: the squared colour distance over sigma_c^2 (isc its inverse) */
struct ColourDist {
    static constexpr bool has_var = false;
    float isc;
    float4 cp;
    __device__ __forceinline__ void centre(float4 c, float) { cp = c; }
    __device__ __forceinline__ float arg(float4 cq) const
    {
        const float dcx = cq.x - cp.x, dcy = cq.y - cp.y, dcz = cq.z - cp.z;
        return (dcx * dcx + dcy * dcy + dcz * dcz) * isc;
    }
};

/* rt_denoise_var: the luminance difference over sigma_lum standard deviations (lum_on == 0: the
   term is off) */
struct LumOverSigma {
    static constexpr bool has_var = true;
    float sigma_lum;
    int lum_on;
    float il, lp;
    __device__ __forceinline__ void centre(float4 c, float g)
    {
        il = lum_on ? 1.0f / (sigma_lum * rt_sqrtf(g) + 1e-8f) : 0.0f;
        lp = lum3(c);
    }
    __device__ __forceinline__ float arg(float4 cq) const { return fabsf(lum3(cq) - lp) * il; }
};

__device__ __forceinline__ float atrous_h(int dx, int dy)
{
    const float k[3] = {0.375f, 0.25f, 0.0625f};
    return k[dx < 0 ? -dx : dx] * k[dy < 0 ? -dy : dy];
}

__device__ __forceinline__ float gauss_k(int dx, int dy)
{
    const float kg[3] = {0.25f, 0.125f, 0.0625f};
    return kg[(dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)];
}

/* One pass, one lane per pixel; a block covers the RT_TILE_BX x RT_TILE_BY tile.  Tap order and
   arithmetic as DESIGN.md §4.9 / §4.11: dy outer, dx inner, a tap outside the frame skipped,
   w = h exp(-((colour + en isn) + ep isp)), acc += c_q w, the variance's += v_q w^2.

   S = 0, the gather form (steps 4 and up): the 25 taps at distance `step` (which only this form
   reads) straight from global memory — the re-reads of lines the neighbours fetch are served by
   the vector L1 / L2, the frame's streams fit the Infinity Cache; a halo of 2 step pixels around
   the tile would not fit LDS from step 8 on.

   S = 1, 2, the staged form (step S): the tile and its halo of 2 S pixels — (32 + 4 S) x (8 + 4 S)
   cells of the streams (48 B a cell: 20,736 B / 30,720 B; with the variance 52 B: 22,464 B /
   33,280 B) — loaded once into LDS, the taps read from there.  The streams are planes of their own:
   a lane row reads consecutive 16-B cells of a float4 plane (conflict-free ds_read_b128) and
   consecutive dwords of the variance plane (32 lanes on 32 banks: conflict-free ds_read_b32);
   interleaved 52-B cells would leave the 16-B reads unaligned.  The unit-distance prefilter stays
   inside the halo (1 <= 2 S).  Cells outside the frame are neither written nor read.  Measured
   25 % / 22 % faster than the gather form at these two steps (profiles/denoise). */
template <int S, class Term>
__device__ __forceinline__ void atrous_pass(const float4 *__restrict__ col, const float *__restrict__ var,
                                            const float4 *__restrict__ feat, float4 *__restrict__ out,
                                            float *__restrict__ out_var, uint32_t W, uint32_t H, int step, Term term,
                                            float isn, float isp)
{
    /* (the gather form's arrays of one cell are unused and take no LDS) */
    constexpr int TW = RT_TILE_BX + 4 * S, TH = RT_TILE_BY + 4 * S, CELLS = S ? TW * TH : 1;
    __shared__ float4 s_c[CELLS], s_p[CELLS], s_n[CELLS];
    __shared__ float s_v[Term::has_var ? CELLS : 1];
    const float4 *__restrict__ pos = feat;
    const float4 *__restrict__ nrm = feat + (size_t)W * H;
    if constexpr (S) {
        const int x0 = (int)(blockIdx.x * RT_TILE_BX) - 2 * S, y0 = (int)(blockIdx.y * RT_TILE_BY) - 2 * S;
        const int tid = (int)(threadIdx.y * RT_TILE_BX + threadIdx.x);
        for (int i = tid; i < TW * TH; i += RT_TILE_BX * RT_TILE_BY) {
            const int gx = x0 + i % TW, gy = y0 + i / TW;
            if (gx >= 0 && gx < (int)W && gy >= 0 && gy < (int)H) {
                const size_t q = (size_t)gy * W + gx;
                s_c[i] = col[q];
                s_p[i] = pos[q];
                s_n[i] = nrm[q];
                if constexpr (Term::has_var) s_v[i] = var[q];
            }
        }
        __syncthreads();
    }
    const int st = S ? S : step;
    const int x = (int)(blockIdx.x * RT_TILE_BX + threadIdx.x);
    const int y = (int)(blockIdx.y * RT_TILE_BY + threadIdx.y);
    if (x >= (int)W || y >= (int)H) return;
    const size_t p = (size_t)y * W + x;
    /* the streams of the pixel (dx, dy) from this one: in the staged tile, or in the frame */
    const float4 *c = S ? s_c : col, *P = S ? s_p : pos, *N = S ? s_n : nrm;
    const float *v = S ? s_v : var;
    const auto at = [&](int dx, int dy) {
        if constexpr (S) return ((int)threadIdx.y + 2 * S + dy) * TW + (int)threadIdx.x + 2 * S + dx;
        else return (size_t)(y + dy) * W + (x + dx);
    };
    const auto inside = [&](int dx, int dy) { return x + dx >= 0 && x + dx < (int)W && y + dy >= 0 && y + dy < (int)H; };
    float g = 0.0f;
    if constexpr (Term::has_var) {
        float ga = 0.0f, gs = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (!inside(dx, dy)) continue;
                const float kg = gauss_k(dx, dy);
                ga += v[at(dx, dy)] * kg;
                gs += kg;
            }
        }
        g = ga / gs;
    }
    const auto p0 = at(0, 0);
    const float4 cp = c[p0], pp = P[p0], np = N[p0];
    term.centre(cp, g);
    float ax = 0.0f, ay = 0.0f, az = 0.0f, av = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (!inside(st * dx, st * dy)) continue;
            const auto q = at(st * dx, st * dy);
            /* all of a tap's loads before its weight: rt_expf branches, and a load after it would
               be issued, and waited for, behind them */
            const float4 cq = c[q], pq = P[q], nq = N[q];
            const float vq = Term::has_var ? v[q] : 0.0f;
            float ep_isp;
            const float en_isn = feat_arg(pq, nq, pp, np, isn, isp, ep_isp);
            const float w = atrous_h(dx, dy) * rt_expf(-((term.arg(cq) + en_isn) + ep_isp));
            ax += cq.x * w;
            ay += cq.y * w;
            az += cq.z * w;
            wsum += w;
            if constexpr (Term::has_var) av += vq * (w * w);
        }
    }
    out[p] = make_float4(ax / wsum, ay / wsum, az / wsum, cp.w);
    if constexpr (Term::has_var)
        if (out_var) out_var[p] = av / (wsum * wsum);
}

/* The six kernels: the pass's instantiations under the names and parameter lists the profiles'
   scripts and the kernel traces know them by. */
#define RT_ATROUS_KERNEL __global__ __launch_bounds__(RT_TILE_BX *RT_TILE_BY) void

RT_ATROUS_KERNEL k_atrous(const float4 *__restrict__ col, const float4 *__restrict__ feat, float4 *__restrict__ out,
                          uint32_t W, uint32_t H, int step, float isc, float isn, float isp)
{
    atrous_pass<0>(col, nullptr, feat, out, nullptr, W, H, step, ColourDist{isc}, isn, isp);
}

template <int S>
RT_ATROUS_KERNEL k_atrous_lds(const float4 *__restrict__ col, const float4 *__restrict__ feat, float4 *__restrict__ out,
                              uint32_t W, uint32_t H, float isc, float isn, float isp)
{
    atrous_pass<S>(col, nullptr, feat, out, nullptr, W, H, S, ColourDist{isc}, isn, isp);
}

RT_ATROUS_KERNEL k_atrous_var(const float4 *__restrict__ col, const float *__restrict__ var,
                              const float4 *__restrict__ feat, float4 *__restrict__ out, float *__restrict__ out_var,
                              uint32_t W, uint32_t H, int step, float sigma_lum, int lum_on, float isn, float isp)
{
    atrous_pass<0>(col, var, feat, out, out_var, W, H, step, LumOverSigma{sigma_lum, lum_on}, isn, isp);
}

template <int S>
RT_ATROUS_KERNEL k_atrous_var_lds(const float4 *__restrict__ col, const float *__restrict__ var,
                                  const float4 *__restrict__ feat, float4 *__restrict__ out,
                                  float *__restrict__ out_var, uint32_t W, uint32_t H, float sigma_lum, int lum_on,
                                  float isn, float isp)
{
    atrous_pass<S>(col, var, feat, out, out_var, W, H, S, LumOverSigma{sigma_lum, lum_on}, isn, isp);
}

} // namespace

int rt_launch_moments(const float *prev_rgba, const float *cur_rgba, float n_cur, const float *mom_in, float *mom_out,
                      uint32_t W, uint32_t H, void *stream)
{
    const uint32_t npx = W * H; /* < 2^28 (the host's frame check) */
    hipLaunchKernelGGL(k_moments, pixel_grid(npx), dim3(kPixelBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(prev_rgba), reinterpret_cast<const float4 *>(cur_rgba), n_cur,
                       1.0f / n_cur, reinterpret_cast<const float4 *>(mom_in), reinterpret_cast<float4 *>(mom_out), npx);
    return (int)hipGetLastError();
}

int rt_launch_moments_tiles(const float *prev_rgba, const float *cur_rgba, float n_cur, const float *mom_in, float *mom_out,
                            const uint32_t *stop, float *len_out, uint32_t W, uint32_t H, void *stream)
{
    const uint32_t npx = W * H; /* < 2^28 (the host's frame check) */
    hipLaunchKernelGGL(k_moments_tiles, pixel_grid(npx), dim3(kPixelBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(prev_rgba), reinterpret_cast<const float4 *>(cur_rgba), n_cur,
                       1.0f / n_cur, reinterpret_cast<const float4 *>(mom_in), reinterpret_cast<float4 *>(mom_out), stop,
                       len_out, W, (W + 7u) / 8u, npx);
    return (int)hipGetLastError();
}

int rt_launch_fold_tiles(const float *sample_rgba, float *acc_rgba, uint32_t *count, const uint32_t *passes, uint32_t pass,
                         const float *mom_in, float *mom_out, float *len_out, uint32_t W, uint32_t H, void *stream)
{
    const uint32_t tw = (W + 7u) / 8u, th = (H + 7u) / 8u, gw = (tw + kHistWaves - 1) / kHistWaves;
    hipLaunchKernelGGL(k_fold_tiles, dim3(gw * th), dim3(kHistBlock), 0, (hipStream_t)stream, /* < 2^22 blocks (the host's frame check) */
                       reinterpret_cast<const float4 *>(sample_rgba), reinterpret_cast<float4 *>(acc_rgba), count, passes, pass,
                       reinterpret_cast<const float4 *>(mom_in), reinterpret_cast<float4 *>(mom_out), len_out, W, H, tw, gw);
    return (int)hipGetLastError();
}

int rt_launch_variance(const float *disp_rgba, const float *mom_rgba, const float *len, const float *feat, float *out_var,
                       uint32_t W, uint32_t H, float isn, float isp, float min_len, void *stream)
{
    hipLaunchKernelGGL(k_variance, tile_grid(W, H), tile_block(), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(disp_rgba), reinterpret_cast<const float4 *>(mom_rgba), len,
                       reinterpret_cast<const float4 *>(feat), out_var, W, H, isn, isp, min_len);
    return (int)hipGetLastError();
}

int rt_launch_atrous(const RtAtrousLaunch &a, void *stream)
{
    const float4 *c4 = reinterpret_cast<const float4 *>(a.col), *f4 = reinterpret_cast<const float4 *>(a.feat);
    float4 *o4 = reinterpret_cast<float4 *>(a.out);
    const auto go = [&](auto kernel, auto... args) {
        hipLaunchKernelGGL(kernel, tile_grid(a.W, a.H), tile_block(), 0, (hipStream_t)stream, args...);
    };
    /* steps 1 and 2 from LDS, the larger ones gathered (the step size decides: profiles/denoise);
       RTMI_ATROUS_LDS (A/B knob, read at every launch, no result bit depends on it): the largest
       step staged, 0 = none */
    const char *knob = getenv("RTMI_ATROUS_LDS");
    const uint32_t lds_max = knob ? (uint32_t)atoi(knob) : 2u;
    const bool staged = a.step <= 2 && a.step <= lds_max;
    if (a.var) {
        if (!staged) go(k_atrous_var, c4, a.var, f4, o4, a.out_var, a.W, a.H, (int)a.step, a.colour, a.lum_on, a.isn, a.isp);
        else if (a.step == 1) go(k_atrous_var_lds<1>, c4, a.var, f4, o4, a.out_var, a.W, a.H, a.colour, a.lum_on, a.isn, a.isp);
        else go(k_atrous_var_lds<2>, c4, a.var, f4, o4, a.out_var, a.W, a.H, a.colour, a.lum_on, a.isn, a.isp);
    } else {
        if (!staged) go(k_atrous, c4, f4, o4, a.W, a.H, (int)a.step, a.colour, a.isn, a.isp);
        else if (a.step == 1) go(k_atrous_lds<1>, c4, f4, o4, a.W, a.H, a.colour, a.isn, a.isp);
        else go(k_atrous_lds<2>, c4, f4, o4, a.W, a.H, a.colour, a.isn, a.isp);
    }
    return (int)hipGetLastError();
}
