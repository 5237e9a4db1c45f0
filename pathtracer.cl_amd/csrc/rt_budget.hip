/*
 * rt_budget.hip — per-tile sample counts on the noise meter's tile map: how many passes each 8x8 tile
 * gets in the next display, and the plane that masks one of those passes (gfx950).
 *
 *   k_tile_budget   one lane per tile: 0 passes for a stopped tile, else 1 and one more for every
 *                   limit the tile's mean relative error lies above; the counts of the tiles by
 *                   passes, their sum and the largest, by one integer atomic a wave and bin
 *   k_pass_mask     one lane per tile: the stop plane (rt_set_tile_stop's sense: 0 = rendered) of pass
 *                   `pass` — a live tile whose passes exceed it is rendered, every other tile is not
 *
 * The fold that goes with them, k_fold_tiles, lies beside the moments' arithmetic in rt_filter.hip.
 * Only comparisons and integers: the results are exact.  Nothing in the reference corresponds to
 * these kernels, and none touches a render's state.
 */
#include <hip/hip_runtime.h>

#include "rt_display_util.h"

namespace {

constexpr int kLimits = RT_BUDGET_MAX_PASSES - 1;
struct Limits {
    float v[kLimits];
};

/* stats: the words of rt_budget_stats (tiles, rounds, tile_passes, reserved, by_passes[0..8]), zeroed
   before the launch.  A NaN mean is above no limit. */
__global__ __launch_bounds__(kPixelBlock) void k_tile_budget(const float2 *__restrict__ tiles, const uint32_t *__restrict__ stop,
                                                             uint32_t n_tiles, uint32_t max_passes, Limits lim,
                                                             uint32_t *__restrict__ passes, uint32_t *stats)
{
    const uint32_t t = blockIdx.x * kPixelBlock + threadIdx.x;
    const bool in = t < n_tiles;
    uint32_t ps = 0u;
    if (in) {
        if (!(stop && stop[t] != 0u)) {
            const float mean = tiles[t].x;
            ps = 1u;
#pragma unroll
            for (int k = 0; k < kLimits; ++k) ps += ((uint32_t)k + 1u < max_passes && mean > lim.v[k]) ? 1u : 0u;
        }
        passes[t] = ps;
    }
    /* (every lane of the wave is here: the lanes beyond the plane count in no bin) */
    uint32_t sum = 0u, top = 0u;
#pragma unroll
    for (uint32_t i = 0; i <= RT_BUDGET_MAX_PASSES; ++i) {
        const uint32_t n = (uint32_t)__popcll(__ballot(in && ps == i));
        if (n && (threadIdx.x & 63u) == 0u) atomicAdd(&stats[4u + i], n);
        sum += i * n;
        top = n ? i : top;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (sum) atomicAdd(&stats[2], sum); /* <= 8 n_tiles < 2^29 */
        if (top) atomicMax(&stats[1], top);
    }
    if (t == 0u) stats[0] = n_tiles;
}

__global__ __launch_bounds__(kPixelBlock) void k_pass_mask(const uint32_t *__restrict__ stop, const uint32_t *__restrict__ passes,
                                                           uint32_t pass, uint32_t n_tiles, uint32_t *__restrict__ mask)
{
    const uint32_t t = blockIdx.x * kPixelBlock + threadIdx.x;
    if (t >= n_tiles) return;
    const bool live = !(stop && stop[t] != 0u) && passes[t] > pass;
    mask[t] = live ? 0u : 1u;
}

} // namespace

int rt_launch_tile_budget(const float *tiles, const uint32_t *stop, uint32_t *passes, uint32_t W, uint32_t H, uint32_t max_passes,
                          const float *limits, uint32_t *stats, void *stream)
{
    const uint32_t tw = (W + 7u) / 8u, th = (H + 7u) / 8u, n_tiles = tw * th; /* W H < 2^28 (the host's frame check): < 2^26 */
    const hipError_t e = hipMemsetAsync(stats, 0, sizeof(rt_budget_stats), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    Limits lim;
    for (int k = 0; k < kLimits; ++k) lim.v[k] = limits[k];
    hipLaunchKernelGGL(k_tile_budget, pixel_grid(n_tiles), dim3(kPixelBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2 *>(tiles), stop, n_tiles, max_passes, lim, passes, stats);
    return (int)hipGetLastError();
}

int rt_launch_pass_mask(const uint32_t *stop, const uint32_t *passes, uint32_t pass, uint32_t W, uint32_t H, uint32_t *mask,
                        void *stream)
{
    const uint32_t tw = (W + 7u) / 8u, th = (H + 7u) / 8u, n_tiles = tw * th;
    hipLaunchKernelGGL(k_pass_mask, pixel_grid(n_tiles), dim3(kPixelBlock), 0, (hipStream_t)stream, stop, passes, pass, n_tiles,
                       mask);
    return (int)hipGetLastError();
}
