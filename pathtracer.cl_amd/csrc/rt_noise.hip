/*
 * rt_noise.hip — the noise meter of the display chain: the relative standard error of the displayed
 * luminance reduced to a histogram, a per-tile map and one figure a host can act on (gfx950;
 * DESIGN.md §4.17).
 *
 *   k_noise_hist   one wave per 8x8 tile, lane j = (y & 7) 8 + (x & 7): per pixel e = sqrt(var) /
 *                  (max(lum, 0) + lum_floor), the bin of e's float bits in the meter's 384 bins
 *                  (§4.15: 16 per octave over 24 octaves from 2^-16), integers only, so the counts are
 *                  exact whatever the order; per tile the sum and the maximum of e by a six-level
 *                  butterfly across the wave's lanes (no LDS, every lane ends with the same bits)
 *   k_noise_stat   one wave: the bin that holds the wanted percentile, its upper edge as the level,
 *                  the pixels in bins that lie wholly at or under the threshold — integers but for
 *                  building two floats from bits
 *
 * Nothing in the reference corresponds to these kernels; their arithmetic is pinned in DESIGN.md
 * §4.17 under the model of include/rt_math.h (no contraction, IEEE division and square root), so
 * that a float32 restatement reproduces every bit.  Neither touches a render's state, and both
 * inputs are only read.
 */
#include <hip/hip_runtime.h>

#include "rt_display_util.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBinsPerLane = kMeterBins / 64;

/* The block histogram (rt_display_util.h: a converged frame is nearly one bin) over groups of
   kHistWaves horizontally adjacent tiles, a tile a wave (a 32 x 8 pixel strip: each of its pixel
   rows is one 512-byte segment of the colour stream).  tiles may be null. */
__global__ __launch_bounds__(kHistBlock) void k_noise_hist(const float4 *__restrict__ rgba, const float *__restrict__ var,
                                                        uint32_t W, uint32_t H, uint32_t tw, uint32_t gw, uint32_t groups,
                                                        float lum_floor, uint32_t *__restrict__ hist,
                                                        float *__restrict__ tiles)
{
    __shared__ uint32_t s_h[kHistWaves * kMeterBins];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *mine = hist_zero(s_h);
    /* (the trip count is the block's: every lane stays in the loop for the ballots and the butterflies) */
    for (uint32_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint32_t ty = g / gw, tx = (g - ty * gw) * kHistWaves + wave;
        const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
        bool valid = false;
        int bin = 0;
        float e = 0.0f;
        if (x < W && y < H) { /* (x < W: tx < tw too) */
            const uint32_t p = y * W + x;
            const float4 c = rgba[p];
            const float v = var[p];
            const float L = lum3(c);
            /* v >= 0 (NaN is not) and finite, L finite; without a branch, so that both loads are in
               flight together (a skipped pixel's quotient is dropped) */
            valid = v >= 0.0f && rt_f2u(v) != RT_INF_BITS && (rt_f2u(L) & 0x7fffffffu) < RT_INF_BITS;
            const float Lp = L > 0.0f ? L : 0.0f;
            const float q = rt_sqrtf(v) / (Lp + lum_floor);
            e = valid ? q : 0.0f;
            bin = meter_bin(rt_f2u(e) & 0x7fffffffu);
        }
        const unsigned long long any = hist_add(mine, valid, bin);
        if (tiles) { /* (uniform) */
            float s = e, m = e;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                s = s + __shfl_xor(s, 1 << k);
                m = rt_maxf(m, __shfl_xor(m, 1 << k));
            }
            if (lane == 0u && tx < tw) {
                const uint32_t n = (uint32_t)__popcll(any);
                float *t = tiles + 2u * (ty * tw + tx);
                t[0] = n ? s / (float)n : 0.0f;
                t[1] = n ? m : 0.0f;
            }
        }
    }
    hist_flush(s_h, hist);
}

/* the sum of v over the wave, in every lane */
__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int k = 0; k < 6; ++k) v += __shfl_xor((unsigned long long)v, 1 << k);
    return v;
}

/* One wave, six consecutive bins a lane: the display waits for this result. */
__global__ __launch_bounds__(64) void k_noise_stat(const uint32_t *__restrict__ hist, uint32_t npx, float percentile,
                                                    float threshold, rt_noise_stats *__restrict__ out)
{
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x) return;
    uint32_t n[kBinsPerLane];
#pragma unroll
    for (int k = 0; k < kBinsPerLane; ++k) n[k] = hist[lane * kBinsPerLane + k]; /* (all in flight together) */
    uint64_t own = 0, under = 0;
#pragma unroll
    for (int k = 0; k < kBinsPerLane; ++k) {
        const int i = (int)lane * kBinsPerLane + k;
        own += n[k];
        /* the bin's upper edge (bin 383's is +INFINITY, which is under no threshold) */
        const bool at_or_under = i < kMeterBins - 1 && meter_bin_top(i) <= threshold;
        under += at_or_under ? n[k] : 0u;
    }
    /* the count before this lane's bins: an inclusive scan of `own` less itself */
    uint64_t incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)incl, d);
        if (lane >= (uint32_t)d) incl += up;
    }
    const uint64_t N = wave_sum(own);
    under = wave_sum(under);
    if (N == 0) {
        if (lane == 0u) {
            out->level = 0.0f;
            out->counted = 0u;
            out->skipped = npx;
            out->below = 0u;
        }
        return;
    }
    uint64_t r = (uint64_t)((double)percentile * (double)N);
    if (r > N - 1) r = N - 1;
    /* the first bin whose running count exceeds r lies in exactly one lane */
    uint64_t c = incl - own;
    if (c <= r && r < incl) {
        int i = (int)lane * kBinsPerLane;
#pragma unroll
        for (int k = 0; k < kBinsPerLane; ++k) {
            c += n[k];
            if (c > r) break;
            ++i;
        }
        out->level = i < kMeterBins - 1 ? meter_bin_top(i) : rt_inff();
        out->counted = (uint32_t)N;
        out->skipped = npx - (uint32_t)N;
        out->below = (uint32_t)under;
    }
}

} // namespace

int rt_launch_noise_hist(const float *rgba, const float *var, uint32_t W, uint32_t H, float lum_floor, uint32_t *hist,
                         float *tiles, void *stream)
{
    const hipError_t e = hipMemsetAsync(hist, 0, kMeterBins * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const uint32_t tw = (W + 7u) / 8u, th = (H + 7u) / 8u, gw = (tw + kHistWaves - 1) / kHistWaves;
    const uint32_t groups = gw * th; /* < 2^28 / 8 + 2^28 / 64 (the host's frame check) */
    hipLaunchKernelGGL(k_noise_hist, hist_grid(groups), dim3(kHistBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4 *>(rgba), var, W, H, tw, gw, groups, lum_floor, hist, tiles);
    return (int)hipGetLastError();
}

int rt_launch_noise_stat(const uint32_t *hist, uint32_t W, uint32_t H, float percentile, float threshold,
                         rt_noise_stats *stats, void *stream)
{
    hipLaunchKernelGGL(k_noise_stat, dim3(1), dim3(64), 0, (hipStream_t)stream, hist, W * H, percentile, threshold, stats);
    return (int)hipGetLastError();
}
