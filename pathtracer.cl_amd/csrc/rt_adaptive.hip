/*
 * rt_adaptive.hip — adaptive sampling on the noise meter's tile map: which 8x8 tiles stop being
 * traced, and the pixel queue's order without them (gfx950).
 *
 *   k_stop_settled   one lane per tile: whether the tile is settled — stopped already, or quiet by
 *                    the meter's (mean, max) pair — into a scratch plane, so that the next kernel
 *                    decides every tile from the plane as it was before the call; the frame gate is
 *                    the call's, or (PER_TILE) the tile's own frames against min_frames (§4.20)
 *   k_tile_len_min   one wave per tile, lane j = (y & 7) 8 + (x & 7): the shortest history length of
 *                    the tile's pixels that met a surface, by a six-level butterfly across the wave
 *                    (§4.20)
 *   k_stop_select    one lane per tile: a live tile whose every neighbour within `dilate` tiles
 *                    inside the frame is settled is stopped (its word becomes the frame count); the
 *                    counts of the live and of the newly stopped tiles by one atomic a wave
 *   k_order_stop     one block: the stable compaction of a tile order to the live tiles, the index
 *                    n_tiles — the first outside the frame, which tile_pixel (rt_kernel_util.h)
 *                    rejects — in every remaining position, and the live count
 *
 * Only comparisons, minima and integers: the results are exact.  Nothing in the reference corresponds to
 * these kernels, and none touches a render's state.
 */
#include <hip/hip_runtime.h>

#include "rt_display_util.h"

namespace {

template <bool PER_TILE>
__global__ __launch_bounds__(kPixelBlock) void k_stop_settled(const float2 *__restrict__ tiles,
                                                              const float *__restrict__ tile_frames,
                                                              const uint32_t *__restrict__ stop, uint32_t n_tiles,
                                                              int quiet_all, float min_frames, float threshold,
                                                              float max_limit, uint32_t *__restrict__ settled)
{
    const uint32_t t = blockIdx.x * kPixelBlock + threadIdx.x;
    if (t >= n_tiles) return;
    const float2 m = tiles[t];
    /* (a NaN of the tile's frames passes no gate) */
    const bool quiet_ok = PER_TILE ? tile_frames[t] >= min_frames : quiet_all != 0;
    /* (a NaN of the map is under no threshold) */
    const bool quiet = quiet_ok && m.x <= threshold && m.y <= max_limit;
    settled[t] = (stop[t] != 0u || quiet) ? 1u : 0u;
}

/* stats: tiles, active, stopped_now, frames (rt_adaptive_stats), the two counts zeroed before the launch */
__global__ __launch_bounds__(kPixelBlock) void k_stop_select(const uint32_t *__restrict__ settled, uint32_t *stop, uint32_t tw,
                                                             uint32_t th, int dilate, uint32_t n_frames, uint32_t *stats)
{
    const uint32_t n_tiles = tw * th;
    const uint32_t t = blockIdx.x * kPixelBlock + threadIdx.x;
    const bool live = t < n_tiles && stop[t] == 0u;
    bool all = live;
    if (live) {
        const int tx = (int)(t % tw), ty = (int)(t / tw);
        for (int dy = -dilate; dy <= dilate; ++dy) {
            const int y = ty + dy;
            if (y < 0 || y >= (int)th) continue;
            for (int dx = -dilate; dx <= dilate; ++dx) {
                const int x = tx + dx;
                if (x < 0 || x >= (int)tw) continue;
                all = all && settled[(uint32_t)y * tw + (uint32_t)x] != 0u;
            }
        }
        if (all) stop[t] = n_frames;
    }
    /* (every lane of the wave is here: the lanes beyond the plane count as neither) */
    const uint32_t n_now = (uint32_t)__popcll(__ballot(live && all));
    const uint32_t n_act = (uint32_t)__popcll(__ballot(live && !all));
    if ((threadIdx.x & 63u) == 0u) {
        if (n_act) atomicAdd(&stats[1], n_act);
        if (n_now) atomicAdd(&stats[2], n_now);
    }
    if (t == 0u) {
        stats[0] = n_tiles;
        stats[3] = n_frames;
    }
}

/* kPixelBlock / 64 tiles a block, a tile a wave: each of a tile's pixel rows is one 32-byte segment of the
   length plane, and with the features one 128-byte line of their normal plane, of which only the id is used.  A lane
   that does not count — outside the frame, beyond the last tile, on no surface — holds +INFINITY, the
   minimum's neutral element; every lane stays for the butterfly.  (-0 reads as +0, like every length that
   is not above 0: the minimum has one set of bits in any order.) */
__global__ __launch_bounds__(kPixelBlock) void k_tile_len_min(const float *__restrict__ len, const float4 *__restrict__ normals,
                                                              uint32_t W, uint32_t H, uint32_t tw, uint32_t n_tiles,
                                                              float *__restrict__ tiles_out)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t t = blockIdx.x * (kPixelBlock / 64u) + wave; /* (uniform over the wave) */
    float v = rt_inff();
    if (t < n_tiles) {
        const uint32_t ty = t / tw, tx = t - ty * tw;
        const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
        if (x < W && y < H) {
            const size_t p = (size_t)y * W + x;
            const float l = len[p];
            const bool counts = !normals || __float_as_int(normals[p].w) != RT_FEAT_NONE;
            if (counts) v = l > 0.0f ? l : 0.0f; /* (a NaN: 0) */
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) v = rt_minf(v, __shfl_xor(v, 1 << k));
    if (lane == 0u && t < n_tiles) tiles_out[t] = v;
}

/* One block walks the order in strips of kOrderStrip entries, kOrderPer consecutive ones a lane (their
   loads in flight together): a lane's live entries, the wave's by a scan across its lanes, the waves'
   through LDS, the strips' in a running count every lane keeps.  At 1920x1080 (32,400 tiles) that is
   8 strips; 2^20 tiles take 256. */
constexpr uint32_t kOrderBlock = 1024, kOrderWaves = kOrderBlock / 64, kOrderPer = 4, kOrderStrip = kOrderBlock * kOrderPer;

__global__ __launch_bounds__(kOrderBlock) void k_order_stop(const uint32_t *__restrict__ base,
                                                            const uint32_t *__restrict__ stop, uint32_t n_tiles,
                                                            uint32_t *__restrict__ out, uint32_t *__restrict__ live_out)
{
    __shared__ uint32_t s_wave[2][kOrderWaves];
    if (blockIdx.x) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t done = 0u; /* the live entries of the strips before this one */
    uint32_t strip = 0u;
    for (uint32_t s0 = 0u; s0 < n_tiles; s0 += kOrderStrip, strip ^= 1u) {
        uint32_t tile[kOrderPer];
        bool keep[kOrderPer];
        uint32_t mine = 0u;
#pragma unroll
        for (uint32_t k = 0; k < kOrderPer; ++k) {
            const uint32_t i = s0 + threadIdx.x * kOrderPer + k;
            tile[k] = i < n_tiles ? (base ? base[i] : i) : n_tiles;
        }
#pragma unroll
        for (uint32_t k = 0; k < kOrderPer; ++k) {
            keep[k] = tile[k] < n_tiles && stop[tile[k]] == 0u;
            mine += keep[k] ? 1u : 0u;
        }
        /* the inclusive scan of `mine` over the wave's lanes */
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (lane == 63u) s_wave[strip][wave] = incl;
        __syncthreads(); /* (the two copies alternate: a wave a strip ahead writes the other one) */
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kOrderWaves; ++w) {
            const uint32_t n = s_wave[strip][w];
            before += w < wave ? n : 0u;
            total += n;
        }
        uint32_t at = done + before + incl - mine; /* <= the entries walked so far: < n_tiles where one is kept */
#pragma unroll
        for (uint32_t k = 0; k < kOrderPer; ++k)
            if (keep[k]) out[at++] = tile[k];
        done += total;
    }
    /* done <= n_tiles: the rest of the n_tiles entries */
    for (uint32_t i = done + threadIdx.x; i < n_tiles; i += kOrderBlock) out[i] = n_tiles;
    if (threadIdx.x == 0u) *live_out = done;
}

} // namespace

int rt_launch_order_stop(const uint32_t *base, const uint32_t *stop, uint32_t n_tiles, uint32_t *out, uint32_t *live,
                         void *stream)
{
    hipLaunchKernelGGL(k_order_stop, dim3(1), dim3(kOrderBlock), 0, (hipStream_t)stream, base, stop, n_tiles, out, live);
    return (int)hipGetLastError();
}

int rt_launch_stop_select(const float *tiles, uint32_t *stop, uint32_t *settled, uint32_t W, uint32_t H, uint32_t n_frames,
                          int quiet_ok, float threshold, float max_limit, uint32_t dilate, uint32_t *stats, void *stream)
{
    const uint32_t tw = (W + 7u) / 8u, th = (H + 7u) / 8u, n_tiles = tw * th; /* W H < 2^28 (the host's frame check): < 2^26 */
    const hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_stop_settled<false>, pixel_grid(n_tiles), dim3(kPixelBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2 *>(tiles), nullptr, stop, n_tiles, quiet_ok, 0.0f, threshold, max_limit,
                       settled);
    hipLaunchKernelGGL(k_stop_select, pixel_grid(n_tiles), dim3(kPixelBlock), 0, (hipStream_t)stream, settled, stop, tw, th,
                       (int)dilate, n_frames, stats);
    return (int)hipGetLastError();
}

int rt_launch_stop_select_frames(const float *tiles, const float *tile_frames, uint32_t *stop, uint32_t *settled, uint32_t W,
                                 uint32_t H, uint32_t n_frames, float min_frames, float threshold, float max_limit,
                                 uint32_t dilate, uint32_t *stats, void *stream)
{
    const uint32_t tw = (W + 7u) / 8u, th = (H + 7u) / 8u, n_tiles = tw * th; /* < 2^26, as above */
    const hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_stop_settled<true>, pixel_grid(n_tiles), dim3(kPixelBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2 *>(tiles), tile_frames, stop, n_tiles, 0, min_frames, threshold, max_limit,
                       settled);
    hipLaunchKernelGGL(k_stop_select, pixel_grid(n_tiles), dim3(kPixelBlock), 0, (hipStream_t)stream, settled, stop, tw, th,
                       (int)dilate, n_frames, stats);
    return (int)hipGetLastError();
}

int rt_launch_tile_len_min(const float *len, const float *normals, float *tiles_out, uint32_t W, uint32_t H, void *stream)
{
    const uint32_t tw = (W + 7u) / 8u, th = (H + 7u) / 8u, n_tiles = tw * th; /* < 2^26, as above */
    constexpr uint32_t kPerBlock = kPixelBlock / 64u;
    hipLaunchKernelGGL(k_tile_len_min, dim3((n_tiles + kPerBlock - 1) / kPerBlock), dim3(kPixelBlock), 0, (hipStream_t)stream, len,
                       reinterpret_cast<const float4 *>(normals), W, H, tw, n_tiles, tiles_out);
    return (int)hipGetLastError();
}
