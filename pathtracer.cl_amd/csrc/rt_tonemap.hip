/*
 * rt_tonemap.hip — the last display stage: meter, expose, tone-map, encode and quantise the shown
 * RGBA32F frame to RGBA8 on the device (gfx950).
 *
 *   k_lum_hist   the meter's histogram: per pixel the bin of its luminance's float bits (exponent and
 *                top four mantissa bits: 16 bins per octave over 24 octaves from 2^-16), integers only,
 *                so the counts are exact whatever the order
 *   k_exposure   one lane: the mean log2 luminance of the kept percentile range at bin centres, the
 *                exposure that brings it to the key, clamped and blended with the previous exposure —
 *                on the device, so that no host sync sits between meter and tone map
 *   k_tonemap    one lane per pixel: exposure, curve (clamp / Reinhard with a white point / ACES fit),
 *                sRGB encoding, 8x8 ordered dither, one dword store
 *
 * Nothing in the reference corresponds to these kernels; their arithmetic is pinned in DESIGN.md
 * §4.15 under the model of include/rt_math.h (no contraction, IEEE division, the pinned pow), so that
 * a float32 restatement reproduces every bit.  None touches a render's state, and the frame is only
 * read.
 */
#include <hip/hip_runtime.h>

#include "rt_display_util.h"

#pragma clang fp contract(off)

namespace {

/* The block histogram (rt_display_util.h) over the frame's pixels, kHistBlock a trip. */
__global__ __launch_bounds__(kHistBlock) void k_lum_hist(const float4 *__restrict__ rgba, uint32_t npx,
                                                         uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_h[kHistWaves * kMeterBins];
    uint32_t *mine = hist_zero(s_h);
    /* (the trip count is the wave's: every lane stays in the loop for the ballots) */
    for (uint32_t base = blockIdx.x * kHistBlock; base < npx; base += gridDim.x * kHistBlock) {
        const uint32_t p = base + threadIdx.x;
        bool counted = false;
        int bin = 0;
        if (p < npx) {
            const float4 c = rgba[p];
            const uint32_t u = rt_f2u(lum3(c));
            counted = u > 0u && u < RT_INF_BITS; /* positive and finite */
            bin = meter_bin(u);
        }
        hist_add(mine, counted, bin);
    }
    hist_flush(s_h, hist);
}

/* One lane, sequential. */
__global__ void k_exposure(const uint32_t *__restrict__ hist, float *exposure_io, float key, float lo, float hi,
                           float e_min, float e_max, float rate)
{
    if (blockIdx.x || threadIdx.x) return;
    const float prev = *exposure_io;
    uint64_t N = 0;
    for (int i = 0; i < kMeterBins; ++i) N += hist[i];
    if (N == 0) {
        *exposure_io = prev > 0.0f ? prev : 1.0f;
        return;
    }
    uint64_t lo_n = (uint64_t)((double)lo * (double)N);
    if (lo_n > N - 1) lo_n = N - 1;
    uint64_t hi_n = (uint64_t)((double)hi * (double)N);
    if (hi_n < lo_n + 1) hi_n = lo_n + 1;
    if (hi_n > N) hi_n = N;
    uint64_t c = 0, S = 0;
    for (int i = 0; i < kMeterBins; ++i) {
        const uint64_t n = hist[i];
        const uint64_t a = c > lo_n ? c : lo_n, b = c + n < hi_n ? c + n : hi_n;
        if (b > a) S += (b - a) * (uint64_t)(2 * i + 1);
        c += n;
    }
    const uint64_t K = hi_n - lo_n;
    const float m = (float)((double)S / (double)(32u * K)) - 16.0f;
    const float Et = rt_minf(rt_maxf(key * rt_powf(2.0f, -m), e_min), e_max);
    const bool fresh = !(prev > 0.0f) || !(prev < rt_inff()); /* none yet, or not finite */
    *exposure_io = fresh ? Et : prev + (Et - prev) * rate;
}

__device__ __forceinline__ uint32_t bayer8(uint32_t x, uint32_t y)
{
    const uint32_t a = x ^ y, b = y;
    return (a & 1u) << 5 | (b & 1u) << 4 | (a & 2u) << 2 | (b & 2u) << 1 | (a & 4u) >> 1 | (b & 4u) >> 2;
}

/* a component after the curve: clamp, encode, clamp, quantise */
__device__ __forceinline__ uint32_t encode8(float v, bool srgb, float d)
{
    v = rt_minf(rt_maxf(v, 0.0f), 1.0f);
    if (srgb) {
        v = (v <= 0.0031308f) ? 12.92f * v : 1.055f * rt_powf(v, 0.41666666f) - 0.055f;
        v = rt_minf(rt_maxf(v, 0.0f), 1.0f);
    }
    const int q = (int)(v * 255.0f + d);
    return (uint32_t)(q < 255 ? q : 255);
}

/* One lane per pixel, one dword store per pixel. */
__global__ __launch_bounds__(kPixelBlock) void k_tonemap(const float4 *__restrict__ rgba, const float *__restrict__ exposure,
                                                 uint32_t *__restrict__ out, uint32_t W, uint32_t npx, uint32_t curve,
                                                 uint32_t srgb, uint32_t dither, float exposure_fixed, float iw)
{
    const uint32_t p = blockIdx.x * kPixelBlock + threadIdx.x;
    if (p >= npx) return;
    const float E = exposure ? *exposure : exposure_fixed;
    const float4 c = rgba[p];
    float v[3] = {c.x * E, c.y * E, c.z * E};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = (v[k] > 0.0f) ? v[k] : 0.0f; /* NaN too */
        v[k] = rt_minf(v[k], 65536.0f);
    }
    if (curve == RT_TONE_REINHARD) {
        const float L = lum3(v[0], v[1], v[2]);
        const float s = (1.0f + L * iw) / (1.0f + L);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] * s;
    } else if (curve == RT_TONE_ACES) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = (v[k] * (2.51f * v[k] + 0.03f)) / (v[k] * (2.43f * v[k] + 0.59f) + 0.14f);
    }
    const float d = dither ? ((float)bayer8(p % W, p / W) + 0.5f) * 0.015625f : 0.5f;
    out[p] = encode8(v[0], srgb != 0u, d) | encode8(v[1], srgb != 0u, d) << 8 | encode8(v[2], srgb != 0u, d) << 16 | 255u << 24;
}

} // namespace

int rt_launch_lum_hist(const float *rgba, uint32_t W, uint32_t H, uint32_t *hist, void *stream)
{
    const uint32_t npx = W * H; /* < 2^28 (the host's frame check) */
    const hipError_t e = hipMemsetAsync(hist, 0, kMeterBins * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_lum_hist, hist_grid((npx + kHistBlock - 1) / kHistBlock), dim3(kHistBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(rgba), npx, hist);
    return (int)hipGetLastError();
}

int rt_launch_exposure(const uint32_t *hist, float *exposure_io, float key, float lo, float hi, float e_min, float e_max,
                       float rate, void *stream)
{
    hipLaunchKernelGGL(k_exposure, dim3(1), dim3(64), 0, (hipStream_t)stream, hist, exposure_io, key, lo, hi, e_min, e_max,
                       rate);
    return (int)hipGetLastError();
}

int rt_launch_tonemap(const RtToneLaunch &a, void *stream)
{
    const uint32_t npx = a.W * a.H; /* < 2^28 */
    hipLaunchKernelGGL(k_tonemap, pixel_grid(npx), dim3(kPixelBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(a.rgba), a.exposure, a.out, a.W, npx, a.curve, a.srgb, a.dither,
                       a.exposure_fixed, a.iw);
    return (int)hipGetLastError();
}
