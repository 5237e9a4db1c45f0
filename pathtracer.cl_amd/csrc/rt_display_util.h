/*
 * rt_display_util.h — what the display kernels' files share: rt_filter.hip (moments, variance, the
 * a-trous passes), rt_temporal.hip (reprojection, merge, trust), rt_tonemap.hip (meter, tone map)
 * rt_noise.hip (the noise meter), rt_adaptive.hip and rt_budget.hip (the rules on its tile map).
 *
 *   lum3                  the luminance of a colour, in the bracketing every restatement depends on
 *   kMeterBin0, meter_bin, meter_bin_top   the meter's 384 bins of a float's bits, and back
 *   kHistBlock, kHistWaves, kHistMaxBlocks, hist_grid, hist_zero, hist_add, hist_flush
 *                         the block histogram over those bins: a copy per wave in LDS
 *   feat_arg              the feature terms of a tap's weight
 *   same_surface_class    whether two surface ids may be compared at all
 *   tile_grid, tile_block, kPixelBlock, pixel_grid   the launch shapes: a lane per pixel of a 2-D
 *                         tile, or of the frame's row-major pixels
 *
 * Only force-inlined functions and constants that two of those kernels use belong here; everything
 * has internal linkage, as in rt_kernel_util.h.  Private to csrc/.
 */
#ifndef RT_DISPLAY_UTIL_H
#define RT_DISPLAY_UTIL_H

#include <hip/hip_runtime.h>

#include "pathtracer_rt.h"
#include "rt_internal.h"
#include "rt_math.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float lum3(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }
__device__ __forceinline__ float lum3(float4 c) { return lum3(c.x, c.y, c.z); }

/* ---- the meter's bins: exponent and top four mantissa bits of a non-negative
   float's bits, 16 bins per octave over 24 octaves from 2^-16; whatever lies under or over them
   counts in the first or the last bin.  Whether a value counts at all, and the masking of a sign
   bit, are the caller's (§4.15 and §4.17 differ there). */
constexpr int kMeterBins = RT_METER_BINS;
constexpr int kMeterBin0 = 1776; /* 2^-16's bits >> 19: (127 - 16) * 16 */

__device__ __forceinline__ int meter_bin(uint32_t bits)
{
    const int b = (int)(bits >> 19) - kMeterBin0;
    return b < 0 ? 0 : (b > kMeterBins - 1 ? kMeterBins - 1 : b);
}

/* bin i's upper edge, the lower edge of bin i + 1 (the last bin has none: it is the caller's +INFINITY) */
__device__ __forceinline__ float meter_bin_top(int i) { return rt_u2f((uint32_t)(i + kMeterBin0 + 1) << 19); }

/* ---- the block histogram of k_lum_hist and k_noise_hist: a persistent grid-stride grid of blocks
   of kHistWaves waves, every wave counting into a copy of its own in LDS (4 x 384 words: 6 KB a
   block).  The kernel declares `__shared__ uint32_t s_h[kHistWaves * kMeterBins]`, takes its wave's
   copy from hist_zero, calls hist_add once per trip of its loop with every lane of the wave in it,
   and ends with hist_flush. */
constexpr int kHistBlock = 256, kHistWaves = kHistBlock / 64;
constexpr uint32_t kHistMaxBlocks = 1024; /* the persistent grid: 4 blocks for each of 256 CUs */

inline dim3 hist_grid(uint32_t items) { return dim3(items < kHistMaxBlocks ? items : kHistMaxBlocks); }

__device__ __forceinline__ uint32_t *hist_zero(uint32_t *s_h)
{
    for (uint32_t i = threadIdx.x; i < kHistWaves * kMeterBins; i += kHistBlock) s_h[i] = 0u;
    __syncthreads();
    return s_h + (threadIdx.x >> 6) * kMeterBins;
}

/* Neighbouring pixels fall into the same bin, so the lanes that share the bin of the wave's first
   counted lane are added by that lane alone, as one LDS atomic of their number (a flat region of the
   frame: one atomic a wave instead of 64 on one address), the others add themselves.  Returns the
   ballot of the counted lanes. */
__device__ __forceinline__ unsigned long long hist_add(uint32_t *mine, bool counted, int bin)
{
    const unsigned long long any = __ballot(counted);
    if (any) {
        const int leader = __ffsll((long long)any) - 1;
        const int b0 = __shfl(bin, leader);
        const unsigned long long same = __ballot(counted && bin == b0);
        if ((int)(threadIdx.x & 63u) == leader) atomicAdd(&mine[b0], (uint32_t)__popcll(same));
        else if (counted && bin != b0) atomicAdd(&mine[bin], 1u);
    }
    return any;
}

/* the block's sum of its copies to global memory, one integer atomic per occupied bin */
__device__ __forceinline__ void hist_flush(const uint32_t *s_h, uint32_t *__restrict__ hist)
{
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (uint32_t)kMeterBins; i += kHistBlock) {
        uint32_t n = 0u;
        for (int w = 0; w < kHistWaves; ++w) n += s_h[w * kMeterBins + i];
        if (n) atomicAdd(&hist[i], n);
    }
}

/* ---- the feature terms of a tap q seen from the centre p: en isn, and ep isp
   through ep_isp — the squared normal difference and the squared distance of q's position from
   p's plane, each times its inverse variance */
__device__ __forceinline__ float feat_arg(float4 pq, float4 nq, float4 pp, float4 np, float isn, float isp, float &ep_isp)
{
    const float dnx = nq.x - np.x, dny = nq.y - np.y, dnz = nq.z - np.z;
    const float en = dnx * dnx + dny * dny + dnz * dnz;
    const float pl = (pq.x - pp.x) * np.x + (pq.y - pp.y) * np.y + (pq.z - pp.z) * np.z;
    const float ep = pl * pl;
    ep_isp = ep * isp;
    return en * isn;
}

/* the surface class: any two triangles of the mesh (ids >= 0), else the same sphere */
__device__ __forceinline__ bool same_surface_class(int idp, int idq) { return (idp >= 0 && idq >= 0) || idp == idq; }

/* ---- launch shapes.  A lane per pixel of RT_TILE_BX x RT_TILE_BY tiles of a W x H frame ... */
inline dim3 tile_grid(uint32_t W, uint32_t H) { return dim3((W + RT_TILE_BX - 1) / RT_TILE_BX, (H + RT_TILE_BY - 1) / RT_TILE_BY); }
inline dim3 tile_block() { return dim3(RT_TILE_BX, RT_TILE_BY); }

/* ... or of the frame's npx pixels in row-major order, kPixelBlock a block */
constexpr uint32_t kPixelBlock = 256;
inline dim3 pixel_grid(uint32_t npx) { return dim3((npx + kPixelBlock - 1) / kPixelBlock); }

} // namespace

#endif /* RT_DISPLAY_UTIL_H */
