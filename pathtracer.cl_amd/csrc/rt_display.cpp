/*
 * rt_display.cpp — the display-side stages of a context (librtmi.so host runtime), with their
 * kernel times:
 *
 *   first-hit features                                        rt_features.hip   DESIGN.md §4.9
 *   the edge-avoiding denoiser                                rt_filter.hip     §4.9
 *   temporal reprojection and merge                           rt_temporal.hip   §4.10
 *   luminance moments, variance, the variance-guided filter   rt_filter.hip     §4.11
 *   the features of a moving mesh in an earlier pose          rt_motion.hip     §4.13
 *   the trust of the carried history                          rt_temporal.hip   §4.14
 *   the meter and the tone map to 8 bits                      rt_tonemap.hip    §4.15
 *   the features of moved spheres on the earlier ones         rt_motion.hip     §4.16
 *   the noise meter                                           rt_noise.hip      §4.17
 *   the stop rule, the masked order, the masked moments       rt_adaptive.hip, rt_filter.hip   §4.18
 *   the fold, the budget rule, the pass mask                  rt_filter.hip, rt_budget.hip     §4.19
 *   the merge, the trust test and the stop rule on per-pixel frame counts   rt_temporal.hip, rt_adaptive.hip   §4.20
 *
 * Every call runs through one driver (AuxCall), which also lays out the staging area of a call on
 * host buffers.
 */
#include <cmath>
#include <initializer_list>
#include <string>

#include "rt_ctx.h"
#include "rt_math.h"

namespace {

/* A feature / denoise call on `st` begins: its events exist, and it is ordered after the context's
   pending render the way a render on another stream is (ev_done), and after an earlier such call. */
int aux_begin(rt_ctx *c, hipStream_t st)
{
    for (rt_ctx::StageTime &t : c->stage_time) {
        HIPCHK(c, t.e0.create());
        HIPCHK(c, t.e1.create());
    }
    HIPCHK(c, c->ev_aux.create(hipEventDisableTiming));
    if (const int r = wait_last_render(c, st)) return r;
    return wait_aux(c, st);
}

/* ... and ends: the next render (rt_render_async) orders itself after ev_aux */
int aux_end(rt_ctx *c, hipStream_t st)
{
    HIPCHK(c, hipEventRecord(c->ev_aux, st));
    c->aux_stream = st;
    return RT_OK;
}

/* growing a display-side buffer: a pending call may still use it */
template <class T> int ensure_dev(rt_ctx *c, DevBuf<T> &buf, size_t n)
{
    if (n <= buf.cap) return RT_OK;
    if (c->aux_stream) HIPCHK(c, hipEventSynchronize(c->ev_aux));
    HIPCHK(c, buf.reserve(n));
    return RT_OK;
}

bool frame_ok(uint32_t W, uint32_t H) { return W && H && (uint64_t)W * H < (1ull << 28); }

/* One plane of a call's staging area (host buffers only): `floats` floats (or 32-bit words),
   uploaded from `up` before the kernels and downloaded to `down` after them (either may be null;
   both for a plane used in place there). */
struct Plane {
    const float *up;
    float *down;
    size_t floats;
};

/* The driver of a display-side call: open (device, stream), begin (the staging area for host
   buffers, aux_begin, the uploads, the stage's first event), the caller's launches, end (the
   second event, the downloads, aux_end). */
struct AuxCall {
    rt_ctx *c;
    RtStage stage;
    hipStream_t st = nullptr;
    bool host = false;
    static constexpr int kMaxPlanes = 6;
    const Plane *planes = nullptr;
    int n_planes = 0;
    size_t off[kMaxPlanes] = {}; /* the planes in declaration order, each 16-byte aligned (float4 streams, px may be odd) */

    int open(void *stream, int flags)
    {
        HIPCHK(c, hipSetDevice(c->device));
        st = stream ? (hipStream_t)stream : c->stream;
        host = !(flags & RT_OUT_DEVICE);
        return RT_OK;
    }
    /* plane i on the device (after begin): in the staging area, or the caller's own buffer */
    float *at(int i, const float *dev) const { return host ? c->d_dn_stage + off[i] : const_cast<float *>(dev); }
    uint32_t *words(int i, const void *dev) const { return reinterpret_cast<uint32_t *>(at(i, static_cast<const float *>(dev))); }
    int begin(const Plane *pl, int n)
    {
        if (n > kMaxPlanes) return fail(c, RT_ERR_ARG, "display call: too many staged planes");
        planes = pl;
        n_planes = n;
        size_t floats = 0;
        for (int i = 0; i < n; ++i) {
            off[i] = floats;
            floats += (pl[i].floats + 3) & ~(size_t)3;
        }
        if (host)
            if (const int r = ensure_dev(c, c->d_dn_stage, floats)) return r;
        if (const int r = aux_begin(c, st)) return r;
        if (host)
            for (int i = 0; i < n_planes; ++i)
                if (planes[i].up)
                    HIPCHK(c, hipMemcpyAsync(c->d_dn_stage + off[i], planes[i].up, planes[i].floats * sizeof(float),
                                             hipMemcpyHostToDevice, st));
        HIPCHK(c, hipEventRecord(c->stage_time[stage].e0, st));
        return RT_OK;
    }
    int end()
    {
        HIPCHK(c, hipEventRecord(c->stage_time[stage].e1, st));
        c->stage_time[stage].have = true;
        if (host)
            for (int i = 0; i < n_planes; ++i)
                if (planes[i].down)
                    HIPCHK(c, hipMemcpyAsync(planes[i].down, c->d_dn_stage + off[i], planes[i].floats * sizeof(float),
                                             hipMemcpyDeviceToHost, st));
        return aux_end(c, st);
    }
};

/* the sync twin of an _async call: its status, then the context's stream drained */
int finish_sync(rt_ctx *c, int r)
{
    if (r != RT_OK) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

/* The kernel times of the stages asked for (a null `ms`: not this one; one at least), once each of
   those has run: none is read before all of them have. */
struct StageOut {
    RtStage stage;
    float *ms;
};
int last_ms(const rt_ctx *c, std::initializer_list<StageOut> want)
{
    if (!c) return RT_ERR_ARG;
    bool any = false;
    for (const StageOut &w : want) {
        if (w.ms && !c->stage_time[w.stage].have) return RT_ERR_STATE;
        any |= w.ms != nullptr;
    }
    if (!any) return RT_ERR_ARG;
    for (const StageOut &w : want) {
        if (!w.ms) continue;
        const rt_ctx::StageTime &t = c->stage_time[w.stage];
        if (hipEventSynchronize(t.e1) != hipSuccess) return RT_ERR_HIP;
        if (hipEventElapsedTime(w.ms, t.e0, t.e1) != hipSuccess) return RT_ERR_HIP;
    }
    return RT_OK;
}

/* 1 / sigma^2 in float: the inverse variance of a weight's term (+INFINITY: 0, the term is off) */
float inv_sq(float sigma) { return 1.0f / (sigma * sigma); }

/* whether [a, a + na) and [b, b + nb) share a byte (addresses of one kind: all host or all device; a
   null buffer shares none) */
bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x && y && x < y + nb && y < x + na;
}

/* Where a meter counts on device buffers: the caller's histogram, or without one the context's own
   (allocated once, never grown).  On host buffers the counts are a plane of the staging area. */
int dev_hist(AuxCall &x, uint32_t *hist_out, DevBuf<uint32_t> &own, uint32_t *&hist)
{
    hist = hist_out;
    if (x.host || hist_out) return RT_OK;
    HIPCHK(x.c, own.reserve(RT_METER_BINS));
    hist = own.p;
    return RT_OK;
}

/* The a-trous passes' ping-pong: pass i reads the previous pass's output (pass 0: the input) and
   writes a scratch buffer, the last one the output — through scratch (and the caller's copy
   afterwards) when that is the buffer it reads (one pass in place). */
float *pass_dst(bool last, float *out, const float *src, DevBuf<float> tmp[2])
{
    return (last && out != src) ? out : tmp[src == tmp[0] ? 1 : 0].p;
}

/* The passes of rt_denoise (in_var null) and of rt_denoise_var, from the scratch buffers to the
   call's end.  pl: the call's planes — colour (filtered in place in the staging area: the last pass
   never reads its destination), the two feature planes, then with in_var the variance plane.
   sigma: sigma_color, its tolerance halving every pass, or sigma_lum. */
int atrous_passes(AuxCall &x, const Plane *pl, const float *in, const float *in_var, const float *feat,
                  float *out, float *out_var, uint32_t W, uint32_t H, uint32_t n, float sigma, int lum_on, float isn,
                  float isp)
{
    rt_ctx *c = x.c;
    const size_t px = (size_t)W * H;
    for (uint32_t k = 0; k < (n > 2 ? 2u : 1u); ++k) { /* (three passes and more alternate between two) */
        if (const int r = ensure_dev(c, c->d_dn_tmp[k], 4 * px)) return r;
        if (in_var)
            if (const int r = ensure_dev(c, c->d_var_tmp[k], px)) return r;
    }
    if (const int r = x.begin(pl, in_var ? 3 : 2)) return r;
    float *dout = x.at(0, out), *dvout = !in_var || (x.host && !out_var) ? nullptr : x.at(2, out_var);
    /* each pass reads the one before it (col, var) and sets its own outputs, step and colour parameter */
    RtAtrousLaunch a = {x.at(0, in), in_var ? x.at(2, in_var) : nullptr, x.at(1, feat), nullptr, nullptr, W, H, 0, 0.0f,
                        lum_on, isn, isp};
    for (uint32_t i = 0; i < n; ++i) {
        const bool last = i + 1 == n;
        a.out = pass_dst(last, dout, a.col, c->d_dn_tmp);
        a.out_var = in_var ? pass_dst(last, dvout, a.var, c->d_var_tmp) : nullptr;
        a.step = 1u << i;
        a.colour = in_var ? sigma : inv_sq(ldexpf(sigma, -(int)i));
        const int e = rt_launch_atrous(a, x.st);
        if (e) return hip_fail(c, (hipError_t)e, "filter kernel launch");
        a.col = a.out;
        a.var = a.out_var;
    }
    if (a.col != dout) HIPCHK(c, hipMemcpyAsync(dout, a.col, 4 * px * sizeof(float), hipMemcpyDeviceToDevice, x.st));
    if (dvout && a.var != dvout) HIPCHK(c, hipMemcpyAsync(dvout, a.var, px * sizeof(float), hipMemcpyDeviceToDevice, x.st));
    return x.end();
}

/* rt_temporal_merge (cur_len null: the frame count is n_cur) and rt_temporal_merge_len (the count is cur_len's,
   per pixel), `who` in the messages */
int temporal_merge(rt_ctx *c, const char *who, const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                   const float *cur_len, float max_history, float *out_rgba, float *out_len, uint32_t W, uint32_t H, int flags,
                   void *stream)
{
    if (!c) return RT_ERR_ARG;
    const std::string w = who;
    if (!hist_rgba || !hist_len || !cur_rgba || !out_rgba || !out_len) return fail(c, RT_ERR_ARG, (w + ": null argument").c_str());
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, (w + ": flags other than RT_OUT_DEVICE").c_str());
    if (!(n_cur >= 1.0f)) return fail(c, RT_ERR_ARG, (w + ": n_cur below 1 or NaN").c_str());
    if (!(max_history >= 1.0f)) return fail(c, RT_ERR_ARG, (w + ": max_history below 1 or NaN").c_str());
    if (out_rgba == cur_rgba) return fail(c, RT_ERR_ARG, (w + ": the output is the current frame's buffer").c_str());
    const size_t px = (size_t)W * H;
    if (overlaps(cur_len, px * sizeof(float), out_rgba, 4 * px * sizeof(float)) ||
        overlaps(cur_len, px * sizeof(float), out_len, px * sizeof(float)))
        return fail(c, RT_ERR_ARG, (w + ": cur_len overlaps an output").c_str());
    AuxCall x = {c, RT_ST_MERGE};
    if (const int r = x.open(stream, flags)) return r;
    /* staged, and merged in place there */
    const Plane pl[] = {{hist_rgba, out_rgba, 4 * px}, {cur_rgba, nullptr, 4 * px}, {hist_len, out_len, px},
                        {cur_len, nullptr, cur_len ? px : 0u}};
    if (const int r = x.begin(pl, 4)) return r;
    const int e = rt_launch_temporal_merge(x.at(0, hist_rgba), x.at(2, hist_len), x.at(1, cur_rgba), n_cur,
                                           cur_len ? x.at(3, cur_len) : nullptr, max_history, x.at(0, out_rgba), x.at(2, out_len),
                                           W, H, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "temporal merge kernel launch");
    return x.end();
}

/* rt_history_trust (cur_len null) and rt_history_trust_len, as temporal_merge */
int history_trust(rt_ctx *c, const char *who, const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                  const float *cur_len, const float *feat, float *out_len, uint32_t W, uint32_t H, const rt_trust_params *prm,
                  int flags, void *stream)
{
    if (!c) return RT_ERR_ARG;
    const std::string w = who;
    if (!hist_rgba || !hist_len || !cur_rgba || !feat || !out_len || !prm) return fail(c, RT_ERR_ARG, (w + ": null argument").c_str());
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, (w + ": flags other than RT_OUT_DEVICE").c_str());
    if (!(n_cur >= 1.0f)) return fail(c, RT_ERR_ARG, (w + ": n_cur below 1 or NaN").c_str());
    if (!(prm->tolerance > 0.0f)) return fail(c, RT_ERR_ARG, (w + ": tolerance is not positive").c_str()); /* <= 0 or NaN */
    if (!(prm->sigma_normal > 0.0f) || !(prm->sigma_plane > 0.0f))
        return fail(c, RT_ERR_ARG, (w + ": a sigma is not positive").c_str()); /* <= 0 or NaN */
    if (out_len == hist_rgba || out_len == cur_rgba || out_len == feat)
        return fail(c, RT_ERR_ARG, (w + ": the output is an input other than hist_len").c_str());
    const size_t px = (size_t)W * H;
    if (overlaps(cur_len, px * sizeof(float), out_len, px * sizeof(float)))
        return fail(c, RT_ERR_ARG, (w + ": cur_len overlaps the output").c_str());
    const bool all = prm->tolerance == rt_inff(); /* everything is trusted: hist_len's bits, no kernel */
    AuxCall x = {c, RT_ST_TRUST};
    if (const int r = x.open(stream, flags)) return r;
    /* the kernel's output lies apart from hist_len, whose neighbours' flags other blocks still read:
       in the staging area a plane of its own, for device buffers in place a scratch plane */
    const bool in_place = !x.host && out_len == hist_len;
    if (in_place && !all)
        if (const int r = ensure_dev(c, c->d_var_tmp[0], px)) return r;
    const Plane pl[] = {{all ? nullptr : hist_rgba, nullptr, 4 * px},
                        {all ? nullptr : cur_rgba, nullptr, 4 * px},
                        {all ? nullptr : feat, nullptr, 8 * px},
                        {hist_len, nullptr, px},
                        {nullptr, out_len, px},
                        {all ? nullptr : cur_len, nullptr, cur_len ? px : 0u}};
    if (const int r = x.begin(pl, 6)) return r;
    const float *dlen = x.at(3, hist_len);
    float *dout = x.at(4, out_len);
    if (all) {
        if (dout != dlen) HIPCHK(c, hipMemcpyAsync(dout, dlen, px * sizeof(float), hipMemcpyDeviceToDevice, x.st));
        return x.end();
    }
    float *dst = in_place ? c->d_var_tmp[0].p : dout;
    const int e = rt_launch_history_trust(x.at(0, hist_rgba), dlen, x.at(1, cur_rgba), n_cur, cur_len ? x.at(5, cur_len) : nullptr,
                                          x.at(2, feat), dst, W, H, prm->tolerance * prm->tolerance, inv_sq(prm->sigma_normal),
                                          inv_sq(prm->sigma_plane), x.st);
    if (e) return hip_fail(c, (hipError_t)e, "history trust kernel launch");
    if (in_place) HIPCHK(c, hipMemcpyAsync(dout, dst, px * sizeof(float), hipMemcpyDeviceToDevice, x.st));
    return x.end();
}

/* rt_tile_stop_select (tile_frames null: the frame gate is n_frames >= min_frames) and rt_tile_stop_select_frames
   (the gate is the tile's own), as temporal_merge */
int stop_select(rt_ctx *c, const char *who, const float *tiles_mean_max, const float *tile_frames, uint32_t *stop_io,
                uint32_t n_frames, rt_adaptive_stats *stats_out, uint32_t W, uint32_t H, const rt_adaptive_params *prm, int flags,
                void *stream)
{
    if (!c) return RT_ERR_ARG;
    const std::string w = who;
    if (!tiles_mean_max || !stop_io || !stats_out || !prm) return fail(c, RT_ERR_ARG, (w + ": null argument").c_str());
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, (w + ": flags other than RT_OUT_DEVICE").c_str());
    if (n_frames == 0) return fail(c, RT_ERR_ARG, (w + ": n_frames is 0").c_str());
    if (!(prm->threshold >= 0.0f)) return fail(c, RT_ERR_ARG, (w + ": threshold negative or NaN").c_str());
    if (!(prm->max_ratio >= 1.0f)) return fail(c, RT_ERR_ARG, (w + ": max_ratio below 1 or NaN").c_str());
    if (prm->dilate > 4) return fail(c, RT_ERR_ARG, (w + ": dilate above 4").c_str());
    const size_t tiles = (size_t)((W + 7u) / 8u) * ((H + 7u) / 8u);
    const size_t tb = 2 * tiles * sizeof(float), sb = tiles * sizeof(uint32_t), qb = sizeof(rt_adaptive_stats);
    if (overlaps(tiles_mean_max, tb, stop_io, sb) || overlaps(tiles_mean_max, tb, stats_out, qb) ||
        overlaps(stop_io, sb, stats_out, qb) || overlaps(tile_frames, sb, stop_io, sb) || overlaps(tile_frames, sb, stats_out, qb))
        return fail(c, RT_ERR_ARG, (w + ": the buffers overlap").c_str());
    /* one float product, formed here; +INFINITY switches the term off (0 x INFINITY would be a NaN) */
    const float max_limit = prm->max_ratio == rt_inff() ? rt_inff() : prm->threshold * prm->max_ratio;
    AuxCall x = {c, RT_ST_STOP_SELECT};
    if (const int r = x.open(stream, flags)) return r;
    if (const int r = ensure_dev(c, c->d_stop_settled, tiles)) return r;
    /* staged: the tile pairs, the plane's words (updated in place there), the stats' words, then the tiles' frames */
    constexpr size_t kStatWords = sizeof(rt_adaptive_stats) / sizeof(float);
    const Plane pl[] = {{tiles_mean_max, nullptr, 2 * tiles},
                        {reinterpret_cast<const float *>(stop_io), reinterpret_cast<float *>(stop_io), tiles},
                        {nullptr, reinterpret_cast<float *>(stats_out), kStatWords},
                        {tile_frames, nullptr, tile_frames ? tiles : 0u}};
    if (const int r = x.begin(pl, 4)) return r;
    const int e = tile_frames
                      ? rt_launch_stop_select_frames(x.at(0, tiles_mean_max), x.at(3, tile_frames), x.words(1, stop_io),
                                                     c->d_stop_settled, W, H, n_frames, (float)prm->min_frames, prm->threshold,
                                                     max_limit, prm->dilate, x.words(2, stats_out), x.st)
                      : rt_launch_stop_select(x.at(0, tiles_mean_max), x.words(1, stop_io), c->d_stop_settled, W, H, n_frames,
                                              n_frames >= prm->min_frames, prm->threshold, max_limit, prm->dilate,
                                              x.words(2, stats_out), x.st);
    if (e) return hip_fail(c, (hipError_t)e, "stop rule kernel launch");
    return x.end();
}

} // namespace

extern "C" {

int rt_render_features_async(rt_ctx *c, float *feat, uint32_t W, uint32_t H, int kernel, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!feat) return fail(c, RT_ERR_ARG, "null feature buffer");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (kernel < RT_KERNEL_SPHERES || kernel > RT_KERNEL_TRIS) return fail(c, RT_ERR_ARG, "unknown kernel");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_render_features: flags other than RT_OUT_DEVICE");
    if (kernel == RT_KERNEL_TRIS && c->n_tris == 0) return fail(c, RT_ERR_NO_MESH, "no mesh set");
    if (kernel != RT_KERNEL_TRIS && c->spheres.empty()) return fail(c, RT_ERR_NO_SCENE, "no spheres set");
    AuxCall x = {c, RT_ST_FEATURES};
    if (const int r = x.open(stream, flags)) return r;
    const size_t px = (size_t)W * H;
    const Plane pl[] = {{nullptr, feat, 8 * px}};
    RtFeatLaunch a{};
    a.cam = frame_camera(c, W);
    a.W = W;
    a.H = H;
    int trav = 0;
    if (kernel == RT_KERNEL_TRIS) {
        trav = trav_kind(c);
        a.nodes = trav_nodes(c);
        a.tris = c->d_tris;
        a.n_tris = c->n_tris;
        a.spill_cap = spill_cap(c);
        if (a.spill_cap) {
            const size_t blocks = ((size_t)W * H + RT_BLOCK - 1) / RT_BLOCK;
            /* (growing it frees the old area: hipFree waits for whatever still runs on it) */
            if (const int r = ensure_spill(c, blocks * RT_BLOCK * a.spill_cap)) return r;
        }
        a.spill = c->d_spill;
    } else {
        a.spheres = c->d_spheres;
        a.n_spheres = (uint32_t)c->spheres.size();
    }
    if (const int r = x.begin(pl, 1)) return r;
    a.feat = x.at(0, feat);
    const int e = rt_launch_features(a, trav, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "feature kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_render_features(rt_ctx *c, float *feat, uint32_t W, uint32_t H, int kernel, int flags)
try {
    return finish_sync(c, rt_render_features_async(c, feat, W, H, kernel, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_denoise_defaults(rt_denoise_params *p)
try {
    if (!p) return RT_ERR_ARG;
    p->iterations = 5;
    p->sigma_color = 2.0f;
    p->sigma_normal = 0.3f;
    p->sigma_plane = 0.1f;
    return RT_OK;
} RT_CATCH(nullptr)

int rt_denoise_async(rt_ctx *c, const float *in, const float *feat, float *out, uint32_t W, uint32_t H,
                     const rt_denoise_params *prm, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!in || !feat || !out || !prm) return fail(c, RT_ERR_ARG, "rt_denoise: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_denoise: flags other than RT_OUT_DEVICE");
    if (prm->iterations < 1 || prm->iterations > 8) return fail(c, RT_ERR_ARG, "rt_denoise: iterations outside 1..8");
    const float sig[3] = {prm->sigma_color, prm->sigma_normal, prm->sigma_plane};
    for (float s : sig)
        if (!(s > 0.0f)) return fail(c, RT_ERR_ARG, "rt_denoise: a sigma is not positive"); /* <= 0 or NaN */
    AuxCall x = {c, RT_ST_DENOISE};
    if (const int r = x.open(stream, flags)) return r;
    const size_t px = (size_t)W * H;
    /* staged: colour (filtered in place there: the last pass never reads its destination) and the
       two feature planes */
    const Plane pl[] = {{in, out, 4 * px}, {feat, nullptr, 8 * px}};
    return atrous_passes(x, pl, in, nullptr, feat, out, nullptr, W, H, prm->iterations, sig[0], 0, inv_sq(sig[1]),
                         inv_sq(sig[2]));
} RT_CATCH(err_of(c))

int rt_denoise(rt_ctx *c, const float *in, const float *feat, float *out, uint32_t W, uint32_t H,
               const rt_denoise_params *prm, int flags)
try {
    return finish_sync(c, rt_denoise_async(c, in, feat, out, W, H, prm, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_last_features_ms(const rt_ctx *c, float *ms)
try {
    return last_ms(c, {{RT_ST_FEATURES, ms}});
} RT_CATCH(err_of(c))

int rt_last_denoise_ms(const rt_ctx *c, float *ms)
try {
    return last_ms(c, {{RT_ST_DENOISE, ms}});
} RT_CATCH(err_of(c))

/* ---- temporal reprojection of the displayed frame ------- */

int rt_reproject_defaults(rt_reproject_params *p)
try {
    if (!p) return RT_ERR_ARG;
    p->plane_tol = 0.01f;
    p->normal_min = 0.9f;
    p->max_history = 32.0f;
    return RT_OK;
} RT_CATCH(nullptr)

int rt_reproject_async(rt_ctx *c, const float *prev_rgba, const float *prev_len, const float *prev_feat,
                       const rt_camera *prev_cam, const float *cur_feat, float *out_rgba, float *out_len, uint32_t W,
                       uint32_t H, const rt_reproject_params *prm, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!prev_rgba || !prev_len || !prev_feat || !prev_cam || !cur_feat || !out_rgba || !out_len || !prm)
        return fail(c, RT_ERR_ARG, "rt_reproject: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_reproject: flags other than RT_OUT_DEVICE");
    if (!(prm->plane_tol >= 0.0f)) return fail(c, RT_ERR_ARG, "rt_reproject: plane_tol negative or NaN");
    if (prm->normal_min != prm->normal_min) return fail(c, RT_ERR_ARG, "rt_reproject: normal_min is NaN");
    if (!(prm->max_history >= 1.0f)) return fail(c, RT_ERR_ARG, "rt_reproject: max_history below 1 or NaN");
    if (out_rgba == prev_rgba || out_len == prev_len)
        return fail(c, RT_ERR_ARG, "rt_reproject: an output is the previous frame's buffer");
    AuxCall x = {c, RT_ST_REPROJECT};
    if (const int r = x.open(stream, flags)) return r;
    const size_t px = (size_t)W * H;
    const Plane pl[] = {{prev_rgba, nullptr, 4 * px}, {prev_feat, nullptr, 8 * px}, {cur_feat, nullptr, 8 * px},
                        {prev_len, nullptr, px},      {nullptr, out_rgba, 4 * px},  {nullptr, out_len, px}};
    if (const int r = x.begin(pl, 6)) return r;
    const int e = rt_launch_reproject(x.at(0, prev_rgba), x.at(3, prev_len), x.at(1, prev_feat), *prev_cam, x.at(2, cur_feat),
                                      x.at(4, out_rgba), x.at(5, out_len), W, H, prm->plane_tol, prm->normal_min,
                                      prm->max_history, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "reprojection kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_reproject(rt_ctx *c, const float *prev_rgba, const float *prev_len, const float *prev_feat,
                 const rt_camera *prev_cam, const float *cur_feat, float *out_rgba, float *out_len, uint32_t W, uint32_t H,
                 const rt_reproject_params *prm, int flags)
try {
    return finish_sync(c, rt_reproject_async(c, prev_rgba, prev_len, prev_feat, prev_cam, cur_feat, out_rgba, out_len, W, H,
                                             prm, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_temporal_merge_async(rt_ctx *c, const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                            float max_history, float *out_rgba, float *out_len, uint32_t W, uint32_t H, int flags,
                            void *stream)
try {
    return temporal_merge(c, "rt_temporal_merge", hist_rgba, hist_len, cur_rgba, n_cur, nullptr, max_history, out_rgba, out_len,
                          W, H, flags, stream);
} RT_CATCH(err_of(c))

int rt_temporal_merge_len_async(rt_ctx *c, const float *hist_rgba, const float *hist_len, const float *cur_rgba,
                                const float *cur_len, float max_history, float *out_rgba, float *out_len, uint32_t W,
                                uint32_t H, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!cur_len) return fail(c, RT_ERR_ARG, "rt_temporal_merge_len: null argument");
    return temporal_merge(c, "rt_temporal_merge_len", hist_rgba, hist_len, cur_rgba, 1.0f, cur_len, max_history, out_rgba,
                          out_len, W, H, flags, stream);
} RT_CATCH(err_of(c))

int rt_temporal_merge_len(rt_ctx *c, const float *hist_rgba, const float *hist_len, const float *cur_rgba, const float *cur_len,
                          float max_history, float *out_rgba, float *out_len, uint32_t W, uint32_t H, int flags)
try {
    return finish_sync(c, rt_temporal_merge_len_async(c, hist_rgba, hist_len, cur_rgba, cur_len, max_history, out_rgba, out_len,
                                                      W, H, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_temporal_merge(rt_ctx *c, const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                      float max_history, float *out_rgba, float *out_len, uint32_t W, uint32_t H, int flags)
try {
    return finish_sync(c, rt_temporal_merge_async(c, hist_rgba, hist_len, cur_rgba, n_cur, max_history, out_rgba, out_len, W,
                                                  H, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_last_reproject_ms(const rt_ctx *c, float *reproject_ms, float *merge_ms)
try {
    return last_ms(c, {{RT_ST_REPROJECT, reproject_ms}, {RT_ST_MERGE, merge_ms}});
} RT_CATCH(err_of(c))

/* ---- lag-adaptive trust of the carried history ----------- */

int rt_trust_defaults(rt_trust_params *p)
try {
    if (!p) return RT_ERR_ARG;
    p->tolerance = 1.5f;
    p->sigma_normal = 0.3f;
    p->sigma_plane = 0.1f;
    return RT_OK;
} RT_CATCH(nullptr)

int rt_history_trust_async(rt_ctx *c, const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                           const float *feat, float *out_len, uint32_t W, uint32_t H, const rt_trust_params *prm, int flags,
                           void *stream)
try {
    return history_trust(c, "rt_history_trust", hist_rgba, hist_len, cur_rgba, n_cur, nullptr, feat, out_len, W, H, prm, flags,
                         stream);
} RT_CATCH(err_of(c))

int rt_history_trust_len_async(rt_ctx *c, const float *hist_rgba, const float *hist_len, const float *cur_rgba,
                               const float *cur_len, const float *feat, float *out_len, uint32_t W, uint32_t H,
                               const rt_trust_params *prm, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!cur_len) return fail(c, RT_ERR_ARG, "rt_history_trust_len: null argument");
    return history_trust(c, "rt_history_trust_len", hist_rgba, hist_len, cur_rgba, 1.0f, cur_len, feat, out_len, W, H, prm, flags,
                         stream);
} RT_CATCH(err_of(c))

int rt_history_trust_len(rt_ctx *c, const float *hist_rgba, const float *hist_len, const float *cur_rgba, const float *cur_len,
                         const float *feat, float *out_len, uint32_t W, uint32_t H, const rt_trust_params *prm, int flags)
try {
    return finish_sync(c, rt_history_trust_len_async(c, hist_rgba, hist_len, cur_rgba, cur_len, feat, out_len, W, H, prm, flags,
                                                     nullptr));
} RT_CATCH(err_of(c))

int rt_history_trust(rt_ctx *c, const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                     const float *feat, float *out_len, uint32_t W, uint32_t H, const rt_trust_params *prm, int flags)
try {
    return finish_sync(c, rt_history_trust_async(c, hist_rgba, hist_len, cur_rgba, n_cur, feat, out_len, W, H, prm, flags,
                                                 nullptr));
} RT_CATCH(err_of(c))

int rt_last_trust_ms(const rt_ctx *c, float *ms)
try {
    return last_ms(c, {{RT_ST_TRUST, ms}});
} RT_CATCH(err_of(c))

/* ---- the features of a moving mesh in an earlier pose ---- */

int rt_warp_features_async(rt_ctx *c, const float *cur_feat, const float *prev_verts, uint32_t n_verts, float *out_feat,
                           uint32_t W, uint32_t H, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!c->n_tris || !c->d_idx || !c->d_pose) return fail(c, RT_ERR_NO_MESH, "no mesh set");
    if (!cur_feat || !prev_verts || !out_feat) return fail(c, RT_ERR_ARG, "rt_warp_features: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (n_verts != c->n_verts) return fail(c, RT_ERR_ARG, "rt_warp_features: the vertex count differs from the mesh's");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_warp_features: flags other than RT_OUT_DEVICE");
    AuxCall x = {c, RT_ST_WARP};
    if (const int r = x.open(stream, flags)) return r;
    const size_t px = (size_t)W * H;
    /* staged: the two feature planes, warped in place there, then the earlier pose */
    const Plane pl[] = {{cur_feat, out_feat, 8 * px}, {prev_verts, nullptr, 3ull * n_verts}};
    if (const int r = x.begin(pl, 2)) return r;
    const int e = rt_launch_warp_features(x.at(0, cur_feat), c->d_idx, c->d_pose, x.at(1, prev_verts), c->n_tris, n_verts,
                                          x.at(0, out_feat), W, H, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "feature warp kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_warp_features(rt_ctx *c, const float *cur_feat, const float *prev_verts, uint32_t n_verts, float *out_feat,
                     uint32_t W, uint32_t H, int flags)
try {
    return finish_sync(c, rt_warp_features_async(c, cur_feat, prev_verts, n_verts, out_feat, W, H, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_last_warp_ms(const rt_ctx *c, float *ms)
try {
    return last_ms(c, {{RT_ST_WARP, ms}});
} RT_CATCH(err_of(c))

/* ---- the features of moved spheres on the earlier spheres ---- */

int rt_warp_features_spheres_async(rt_ctx *c, const float *cur_feat, const rt_sphere *prev_spheres, uint32_t n_prev,
                                   float *out_feat, uint32_t W, uint32_t H, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (c->spheres.empty() || !c->d_spheres) return fail(c, RT_ERR_NO_SCENE, "no spheres set");
    if (!cur_feat || !out_feat) return fail(c, RT_ERR_ARG, "rt_warp_features_spheres: null feature buffer");
    if (n_prev && !prev_spheres) return fail(c, RT_ERR_ARG, "rt_warp_features_spheres: null earlier spheres");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_warp_features_spheres: flags other than RT_OUT_DEVICE");
    const size_t px = (size_t)W * H;
    /* out_feat is cur_feat exactly, or apart from both inputs */
    const size_t feat_bytes = 8 * px * sizeof(float), prev_bytes = (size_t)n_prev * sizeof(rt_sphere);
    if ((out_feat != cur_feat && overlaps(out_feat, feat_bytes, cur_feat, feat_bytes)) ||
        (n_prev && overlaps(out_feat, feat_bytes, prev_spheres, prev_bytes)))
        return fail(c, RT_ERR_ARG, "rt_warp_features_spheres: the output overlaps an input other than exactly cur_feat");
    AuxCall x = {c, RT_ST_WARP_SPH};
    if (const int r = x.open(stream, flags)) return r;
    /* staged: the two feature planes, warped in place there, then the earlier spheres (20 words each) */
    constexpr size_t kSphereFloats = sizeof(rt_sphere) / sizeof(float);
    const float *prev = n_prev ? reinterpret_cast<const float *>(prev_spheres) : nullptr;
    const Plane pl[] = {{cur_feat, out_feat, 8 * px}, {prev, nullptr, kSphereFloats * n_prev}};
    if (const int r = x.begin(pl, 2)) return r;
    const int e = rt_launch_warp_features_spheres(x.at(0, cur_feat), c->d_spheres, (uint32_t)c->spheres.size(),
                                                  prev ? reinterpret_cast<const rt_sphere *>(x.at(1, prev)) : nullptr, n_prev,
                                                  x.at(0, out_feat), W, H, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "sphere feature warp kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_warp_features_spheres(rt_ctx *c, const float *cur_feat, const rt_sphere *prev_spheres, uint32_t n_prev, float *out_feat,
                             uint32_t W, uint32_t H, int flags)
try {
    return finish_sync(c, rt_warp_features_spheres_async(c, cur_feat, prev_spheres, n_prev, out_feat, W, H, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_last_sphere_warp_ms(const rt_ctx *c, float *ms)
try {
    return last_ms(c, {{RT_ST_WARP_SPH, ms}});
} RT_CATCH(err_of(c))

/* ---- variance-guided display filter --------------------- */

int rt_denoise_var_defaults(rt_denoise_var_params *p)
try {
    if (!p) return RT_ERR_ARG;
    p->iterations = 5;
    p->sigma_lum = 4.0f;
    p->sigma_normal = 0.3f;
    p->sigma_plane = 0.1f;
    p->min_len = 4.0f;
    return RT_OK;
} RT_CATCH(nullptr)

int rt_moments_accumulate_async(rt_ctx *c, const float *prev_rgba, const float *cur_rgba, float n_cur,
                                const float *mom_in, float *mom_out, uint32_t W, uint32_t H, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!(n_cur >= 1.0f)) return fail(c, RT_ERR_ARG, "rt_moments_accumulate: n_cur below 1 or NaN");
    const bool first = n_cur == 1.0f; /* the view's first frame: no history is read */
    if (!cur_rgba || !mom_out || (!first && (!prev_rgba || !mom_in)))
        return fail(c, RT_ERR_ARG, "rt_moments_accumulate: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_moments_accumulate: flags other than RT_OUT_DEVICE");
    if (mom_out == prev_rgba || mom_out == cur_rgba)
        return fail(c, RT_ERR_ARG, "rt_moments_accumulate: the output is an accumulation buffer");
    AuxCall x = {c, RT_ST_MOMENTS};
    if (const int r = x.open(stream, flags)) return r;
    const size_t px = (size_t)W * H;
    /* staged: cur, prev, then the moments, accumulated in place there */
    const Plane pl[] = {{cur_rgba, nullptr, 4 * px},
                        {first ? nullptr : prev_rgba, nullptr, 4 * px},
                        {first ? nullptr : mom_in, mom_out, 4 * px}};
    if (const int r = x.begin(pl, 3)) return r;
    const int e = rt_launch_moments(x.at(1, prev_rgba), x.at(0, cur_rgba), n_cur, x.at(2, mom_in), x.at(2, mom_out), W, H, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "moments kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_moments_accumulate(rt_ctx *c, const float *prev_rgba, const float *cur_rgba, float n_cur, const float *mom_in,
                          float *mom_out, uint32_t W, uint32_t H, int flags)
try {
    return finish_sync(c, rt_moments_accumulate_async(c, prev_rgba, cur_rgba, n_cur, mom_in, mom_out, W, H, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_moments_accumulate_tiles_async(rt_ctx *c, const float *prev_rgba, const float *cur_rgba, float n_cur,
                                      const float *mom_in, float *mom_out, const uint32_t *stop, float *len_out, uint32_t W,
                                      uint32_t H, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!(n_cur >= 1.0f)) return fail(c, RT_ERR_ARG, "rt_moments_accumulate_tiles: n_cur below 1 or NaN");
    const bool first = n_cur == 1.0f;
    if (!cur_rgba || !mom_out || !stop || !len_out || (!first && (!prev_rgba || !mom_in)))
        return fail(c, RT_ERR_ARG, "rt_moments_accumulate_tiles: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_moments_accumulate_tiles: flags other than RT_OUT_DEVICE");
    if (mom_out == prev_rgba || mom_out == cur_rgba)
        return fail(c, RT_ERR_ARG, "rt_moments_accumulate_tiles: the output is an accumulation buffer");
    const size_t px = (size_t)W * H, tiles = (size_t)((W + 7u) / 8u) * ((H + 7u) / 8u);
    /* len_out apart from everything else, the plane apart from the moments written */
    const struct {
        const void *p;
        size_t bytes;
    } buf[] = {{prev_rgba, 4 * px * sizeof(float)}, {cur_rgba, 4 * px * sizeof(float)}, {mom_in, 4 * px * sizeof(float)},
               {mom_out, 4 * px * sizeof(float)},   {stop, tiles * sizeof(uint32_t)}};
    for (const auto &b : buf)
        if (overlaps(len_out, px * sizeof(float), b.p, b.bytes))
            return fail(c, RT_ERR_ARG, "rt_moments_accumulate_tiles: len_out overlaps another buffer");
    if (overlaps(stop, tiles * sizeof(uint32_t), mom_out, 4 * px * sizeof(float)))
        return fail(c, RT_ERR_ARG, "rt_moments_accumulate_tiles: the stop plane overlaps the output");
    AuxCall x = {c, RT_ST_MOMENTS};
    if (const int r = x.open(stream, flags)) return r;
    /* staged: cur, prev, the moments (accumulated in place there; without mom_in the output's own
       contents, which a stopped tile keeps), the plane's words, then the lengths */
    const Plane pl[] = {{cur_rgba, nullptr, 4 * px},
                        {first ? nullptr : prev_rgba, nullptr, 4 * px},
                        {mom_in ? mom_in : mom_out, mom_out, 4 * px},
                        {reinterpret_cast<const float *>(stop), nullptr, tiles},
                        {nullptr, len_out, px}};
    if (const int r = x.begin(pl, 5)) return r;
    const float *din = mom_in || x.host ? x.at(2, mom_in) : nullptr;
    const int e = rt_launch_moments_tiles(x.at(1, prev_rgba), x.at(0, cur_rgba), n_cur, din, x.at(2, mom_out), x.words(3, stop),
                                          x.at(4, len_out), W, H, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "masked moments kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_moments_accumulate_tiles(rt_ctx *c, const float *prev_rgba, const float *cur_rgba, float n_cur, const float *mom_in,
                                float *mom_out, const uint32_t *stop, float *len_out, uint32_t W, uint32_t H, int flags)
try {
    return finish_sync(c, rt_moments_accumulate_tiles_async(c, prev_rgba, cur_rgba, n_cur, mom_in, mom_out, stop, len_out, W,
                                                            H, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_variance_async(rt_ctx *c, const float *disp_rgba, const float *mom_rgba, const float *len, const float *feat,
                      float *out_var, uint32_t W, uint32_t H, const rt_denoise_var_params *prm, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!disp_rgba || !mom_rgba || !len || !feat || !out_var || !prm) return fail(c, RT_ERR_ARG, "rt_variance: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_variance: flags other than RT_OUT_DEVICE");
    if (!(prm->min_len >= 2.0f)) return fail(c, RT_ERR_ARG, "rt_variance: min_len below 2 or NaN");
    if (!(prm->sigma_normal > 0.0f) || !(prm->sigma_plane > 0.0f))
        return fail(c, RT_ERR_ARG, "rt_variance: a sigma is not positive"); /* <= 0 or NaN */
    AuxCall x = {c, RT_ST_VARIANCE};
    if (const int r = x.open(stream, flags)) return r;
    const size_t px = (size_t)W * H;
    const Plane pl[] = {{disp_rgba, nullptr, 4 * px}, {mom_rgba, nullptr, 4 * px}, {feat, nullptr, 8 * px},
                        {len, nullptr, px},           {nullptr, out_var, px}};
    if (const int r = x.begin(pl, 5)) return r;
    const int e = rt_launch_variance(x.at(0, disp_rgba), x.at(1, mom_rgba), x.at(3, len), x.at(2, feat), x.at(4, out_var), W, H,
                                     inv_sq(prm->sigma_normal), inv_sq(prm->sigma_plane), prm->min_len, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "variance kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_variance(rt_ctx *c, const float *disp_rgba, const float *mom_rgba, const float *len, const float *feat,
                float *out_var, uint32_t W, uint32_t H, const rt_denoise_var_params *prm, int flags)
try {
    return finish_sync(c, rt_variance_async(c, disp_rgba, mom_rgba, len, feat, out_var, W, H, prm, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_denoise_var_async(rt_ctx *c, const float *in, const float *in_var, const float *feat, float *out, float *out_var,
                         uint32_t W, uint32_t H, const rt_denoise_var_params *prm, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!in || !in_var || !feat || !out || !prm) return fail(c, RT_ERR_ARG, "rt_denoise_var: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_denoise_var: flags other than RT_OUT_DEVICE");
    if (prm->iterations < 1 || prm->iterations > 8) return fail(c, RT_ERR_ARG, "rt_denoise_var: iterations outside 1..8");
    const float sig[3] = {prm->sigma_lum, prm->sigma_normal, prm->sigma_plane};
    for (float s : sig)
        if (!(s > 0.0f)) return fail(c, RT_ERR_ARG, "rt_denoise_var: a sigma is not positive"); /* <= 0 or NaN */
    const int lum_on = sig[0] < rt_inff(); /* +INFINITY: the luminance term is off (inf * 0 would be a NaN) */
    AuxCall x = {c, RT_ST_DENOISE_VAR};
    if (const int r = x.open(stream, flags)) return r;
    const size_t px = (size_t)W * H;
    /* staged: colour, the two feature planes, then the variance plane; filtered in place there
       (the last pass never reads its destination) */
    const Plane pl[] = {{in, out, 4 * px}, {feat, nullptr, 8 * px}, {in_var, out_var, px}};
    return atrous_passes(x, pl, in, in_var, feat, out, out_var, W, H, prm->iterations, sig[0], lum_on, inv_sq(sig[1]),
                         inv_sq(sig[2]));
} RT_CATCH(err_of(c))

int rt_denoise_var(rt_ctx *c, const float *in, const float *in_var, const float *feat, float *out, float *out_var,
                   uint32_t W, uint32_t H, const rt_denoise_var_params *prm, int flags)
try {
    return finish_sync(c, rt_denoise_var_async(c, in, in_var, feat, out, out_var, W, H, prm, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_last_variance_ms(const rt_ctx *c, float *moments_ms, float *variance_ms, float *denoise_var_ms)
try {
    return last_ms(c, {{RT_ST_MOMENTS, moments_ms}, {RT_ST_VARIANCE, variance_ms}, {RT_ST_DENOISE_VAR, denoise_var_ms}});
} RT_CATCH(err_of(c))

/* ---- tone-mapped 8-bit display output with auto-exposure ---- */

int rt_tonemap_defaults(rt_tonemap_params *p)
try {
    if (!p) return RT_ERR_ARG;
    p->curve = RT_TONE_ACES;
    p->srgb = 1;
    p->dither = 1;
    p->exposure = 1.0f;
    p->white = 4.0f;
    return RT_OK;
} RT_CATCH(nullptr)

int rt_meter_defaults(rt_meter_params *p)
try {
    if (!p) return RT_ERR_ARG;
    p->key = 0.18f;
    p->lo = 0.10f;
    p->hi = 0.95f;
    p->e_min = 0.00390625f; /* 2^-8 */
    p->e_max = 4096.0f;     /* 2^12 */
    p->rate = 1.0f;
    return RT_OK;
} RT_CATCH(nullptr)

int rt_meter_exposure_async(rt_ctx *c, const float *rgba, float *exposure_io, uint32_t *hist_out, uint32_t W, uint32_t H,
                            const rt_meter_params *prm, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!rgba || !exposure_io || !prm) return fail(c, RT_ERR_ARG, "rt_meter_exposure: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_meter_exposure: flags other than RT_OUT_DEVICE");
    if (!(prm->key > 0.0f)) return fail(c, RT_ERR_ARG, "rt_meter_exposure: key is not positive"); /* <= 0 or NaN */
    if (!(prm->lo >= 0.0f && prm->lo < 1.0f)) return fail(c, RT_ERR_ARG, "rt_meter_exposure: lo outside [0, 1)");
    if (!(prm->hi > prm->lo && prm->hi <= 1.0f)) return fail(c, RT_ERR_ARG, "rt_meter_exposure: hi outside (lo, 1]");
    if (!(prm->e_min > 0.0f) || !(prm->e_min <= prm->e_max))
        return fail(c, RT_ERR_ARG, "rt_meter_exposure: e_min is not positive, or above e_max");
    if (!(prm->rate > 0.0f && prm->rate <= 1.0f)) return fail(c, RT_ERR_ARG, "rt_meter_exposure: rate outside (0, 1]");
    AuxCall x = {c, RT_ST_METER};
    if (const int r = x.open(stream, flags)) return r;
    const size_t px = (size_t)W * H;
    /* staged: the frame, the exposure, then the counts (words where the other planes hold floats) */
    const Plane pl[] = {{rgba, nullptr, 4 * px}, {exposure_io, exposure_io, 1}, {nullptr, reinterpret_cast<float *>(hist_out), RT_METER_BINS}};
    uint32_t *hist;
    if (const int r = dev_hist(x, hist_out, c->d_meter_hist, hist)) return r;
    if (const int r = x.begin(pl, 3)) return r;
    hist = x.words(2, hist);
    int e = rt_launch_lum_hist(x.at(0, rgba), W, H, hist, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "meter histogram kernel launch");
    e = rt_launch_exposure(hist, x.at(1, exposure_io), prm->key, prm->lo, prm->hi, prm->e_min, prm->e_max, prm->rate, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "exposure kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_meter_exposure(rt_ctx *c, const float *rgba, float *exposure_io, uint32_t *hist_out, uint32_t W, uint32_t H,
                      const rt_meter_params *prm, int flags)
try {
    return finish_sync(c, rt_meter_exposure_async(c, rgba, exposure_io, hist_out, W, H, prm, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_tonemap_async(rt_ctx *c, const float *rgba, const float *exposure, uint32_t *out, uint32_t W, uint32_t H,
                     const rt_tonemap_params *prm, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!rgba || !out || !prm) return fail(c, RT_ERR_ARG, "rt_tonemap: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_tonemap: flags other than RT_OUT_DEVICE");
    if (prm->curve > RT_TONE_ACES) return fail(c, RT_ERR_ARG, "rt_tonemap: unknown curve");
    if (!(prm->white > 0.0f)) return fail(c, RT_ERR_ARG, "rt_tonemap: white is not positive"); /* <= 0 or NaN */
    if (!exposure && !(prm->exposure > 0.0f)) return fail(c, RT_ERR_ARG, "rt_tonemap: exposure is not positive");
    AuxCall x = {c, RT_ST_TONEMAP};
    if (const int r = x.open(stream, flags)) return r;
    const size_t px = (size_t)W * H;
    /* staged: the frame, the 8-bit frame (words), then the exposure */
    const Plane pl[] = {{rgba, nullptr, 4 * px}, {nullptr, reinterpret_cast<float *>(out), px}, {exposure, nullptr, 1}};
    if (const int r = x.begin(pl, 3)) return r;
    const RtToneLaunch a = {x.at(0, rgba),
                            exposure ? x.at(2, exposure) : nullptr,
                            x.words(1, out),
                            W,
                            H,
                            prm->curve,
                            prm->srgb,
                            prm->dither,
                            prm->exposure,
                            inv_sq(prm->white)};
    const int e = rt_launch_tonemap(a, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "tone-map kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_tonemap(rt_ctx *c, const float *rgba, const float *exposure, uint32_t *out, uint32_t W, uint32_t H,
               const rt_tonemap_params *prm, int flags)
try {
    return finish_sync(c, rt_tonemap_async(c, rgba, exposure, out, W, H, prm, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_last_tonemap_ms(const rt_ctx *c, float *meter_ms, float *tonemap_ms)
try {
    return last_ms(c, {{RT_ST_METER, meter_ms}, {RT_ST_TONEMAP, tonemap_ms}});
} RT_CATCH(err_of(c))

/* ---- the noise meter ------------------------------------- */

int rt_noise_defaults(rt_noise_params *p)
try {
    if (!p) return RT_ERR_ARG;
    p->percentile = 0.95f;
    p->threshold = 0.05f;
    p->lum_floor = 1e-3f;
    return RT_OK;
} RT_CATCH(nullptr)

int rt_noise_meter_async(rt_ctx *c, const float *rgba, const float *var, rt_noise_stats *stats_out, float *tiles_out,
                         uint32_t *hist_out, uint32_t W, uint32_t H, const rt_noise_params *prm, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!rgba || !var || !stats_out || !prm) return fail(c, RT_ERR_ARG, "rt_noise_meter: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_noise_meter: flags other than RT_OUT_DEVICE");
    if (!(prm->percentile > 0.0f && prm->percentile <= 1.0f)) return fail(c, RT_ERR_ARG, "rt_noise_meter: percentile outside (0, 1]");
    if (!(prm->threshold >= 0.0f)) return fail(c, RT_ERR_ARG, "rt_noise_meter: threshold negative or NaN");
    if (!(prm->lum_floor > 0.0f && prm->lum_floor < rt_inff()))
        return fail(c, RT_ERR_ARG, "rt_noise_meter: lum_floor is not positive and finite");
    const size_t px = (size_t)W * H, tiles = (size_t)((W + 7u) / 8u) * ((H + 7u) / 8u);
    /* every output apart from both inputs and from the other outputs (a null one is not there) */
    const struct {
        const void *p;
        size_t bytes;
    } buf[] = {{rgba, 4 * px * sizeof(float)},          {var, px * sizeof(float)},
               {stats_out, sizeof(rt_noise_stats)},     {tiles_out, 2 * tiles * sizeof(float)},
               {hist_out, RT_METER_BINS * sizeof(uint32_t)}};
    for (int o = 2; o < 5; ++o)
        for (int i = 0; i < o; ++i)
            if (overlaps(buf[o].p, buf[o].bytes, buf[i].p, buf[i].bytes))
                return fail(c, RT_ERR_ARG, "rt_noise_meter: an output overlaps an input or another output");
    AuxCall x = {c, RT_ST_NOISE};
    if (const int r = x.open(stream, flags)) return r;
    /* staged: the frame, the variance plane, then the words of the stats, the counts and the tile pairs */
    constexpr size_t kStatWords = sizeof(rt_noise_stats) / sizeof(float);
    const Plane pl[] = {{rgba, nullptr, 4 * px},
                        {var, nullptr, px},
                        {nullptr, reinterpret_cast<float *>(stats_out), kStatWords},
                        {nullptr, reinterpret_cast<float *>(hist_out), RT_METER_BINS},
                        {nullptr, tiles_out, 2 * tiles}};
    uint32_t *hist;
    if (const int r = dev_hist(x, hist_out, c->d_noise_hist, hist)) return r;
    if (const int r = x.begin(pl, 5)) return r;
    hist = x.words(3, hist);
    float *dtiles = tiles_out ? x.at(4, tiles_out) : nullptr;
    int e = rt_launch_noise_hist(x.at(0, rgba), x.at(1, var), W, H, prm->lum_floor, hist, dtiles, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "noise histogram kernel launch");
    e = rt_launch_noise_stat(hist, W, H, prm->percentile, prm->threshold,
                             reinterpret_cast<rt_noise_stats *>(x.words(2, stats_out)), x.st);
    if (e) return hip_fail(c, (hipError_t)e, "noise statistic kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_noise_meter(rt_ctx *c, const float *rgba, const float *var, rt_noise_stats *stats_out, float *tiles_out,
                   uint32_t *hist_out, uint32_t W, uint32_t H, const rt_noise_params *prm, int flags)
try {
    return finish_sync(c, rt_noise_meter_async(c, rgba, var, stats_out, tiles_out, hist_out, W, H, prm, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_last_noise_ms(const rt_ctx *c, float *ms)
try {
    return last_ms(c, {{RT_ST_NOISE, ms}});
} RT_CATCH(err_of(c))

/* ---- adaptive sampling on the tile map (rt_set_tile_stop: rt_render.cpp) ---- */

int rt_adaptive_defaults(rt_adaptive_params *p)
try {
    if (!p) return RT_ERR_ARG;
    p->threshold = 0.05f;
    p->max_ratio = 4.0f;
    p->min_frames = 16;
    p->dilate = 1;
    return RT_OK;
} RT_CATCH(nullptr)

int rt_tile_stop_select_async(rt_ctx *c, const float *tiles_mean_max, uint32_t *stop_io, uint32_t n_frames,
                              rt_adaptive_stats *stats_out, uint32_t W, uint32_t H, const rt_adaptive_params *prm, int flags,
                              void *stream)
try {
    return stop_select(c, "rt_tile_stop_select", tiles_mean_max, nullptr, stop_io, n_frames, stats_out, W, H, prm, flags, stream);
} RT_CATCH(err_of(c))

int rt_tile_stop_select_frames_async(rt_ctx *c, const float *tiles_mean_max, const float *tile_frames, uint32_t *stop_io,
                                     uint32_t n_frames, rt_adaptive_stats *stats_out, uint32_t W, uint32_t H,
                                     const rt_adaptive_params *prm, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!tile_frames) return fail(c, RT_ERR_ARG, "rt_tile_stop_select_frames: null argument");
    return stop_select(c, "rt_tile_stop_select_frames", tiles_mean_max, tile_frames, stop_io, n_frames, stats_out, W, H, prm, flags,
                       stream);
} RT_CATCH(err_of(c))

int rt_tile_stop_select_frames(rt_ctx *c, const float *tiles_mean_max, const float *tile_frames, uint32_t *stop_io,
                               uint32_t n_frames, rt_adaptive_stats *stats_out, uint32_t W, uint32_t H,
                               const rt_adaptive_params *prm, int flags)
try {
    return finish_sync(c, rt_tile_stop_select_frames_async(c, tiles_mean_max, tile_frames, stop_io, n_frames, stats_out, W, H, prm,
                                                           flags, nullptr));
} RT_CATCH(err_of(c))

int rt_tile_len_min_async(rt_ctx *c, const float *len, const float *feat, float *tiles_out, uint32_t W, uint32_t H, int flags,
                          void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!len || !tiles_out) return fail(c, RT_ERR_ARG, "rt_tile_len_min: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_tile_len_min: flags other than RT_OUT_DEVICE");
    const size_t px = (size_t)W * H, tiles = (size_t)((W + 7u) / 8u) * ((H + 7u) / 8u);
    if (overlaps(tiles_out, tiles * sizeof(float), len, px * sizeof(float)) ||
        overlaps(tiles_out, tiles * sizeof(float), feat, 8 * px * sizeof(float)))
        return fail(c, RT_ERR_ARG, "rt_tile_len_min: the output overlaps an input");
    AuxCall x = {c, RT_ST_TILE_LEN};
    if (const int r = x.open(stream, flags)) return r;
    /* staged: the lengths, the normal plane of the features (the position plane is not read), then the tiles */
    const Plane pl[] = {{len, nullptr, px}, {feat ? feat + 4 * px : nullptr, nullptr, feat ? 4 * px : 0u}, {nullptr, tiles_out, tiles}};
    if (const int r = x.begin(pl, 3)) return r;
    const int e = rt_launch_tile_len_min(x.at(0, len), feat ? x.at(1, feat + 4 * px) : nullptr, x.at(2, tiles_out), W, H, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "tile length kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_tile_len_min(rt_ctx *c, const float *len, const float *feat, float *tiles_out, uint32_t W, uint32_t H, int flags)
try {
    return finish_sync(c, rt_tile_len_min_async(c, len, feat, tiles_out, W, H, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_last_tile_len_ms(const rt_ctx *c, float *ms)
try {
    return last_ms(c, {{RT_ST_TILE_LEN, ms}});
} RT_CATCH(err_of(c))

int rt_tile_stop_select(rt_ctx *c, const float *tiles_mean_max, uint32_t *stop_io, uint32_t n_frames,
                        rt_adaptive_stats *stats_out, uint32_t W, uint32_t H, const rt_adaptive_params *prm, int flags)
try {
    return finish_sync(c, rt_tile_stop_select_async(c, tiles_mean_max, stop_io, n_frames, stats_out, W, H, prm, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_tile_stop_order_async(rt_ctx *c, const uint32_t *base, const uint32_t *stop, uint32_t n_tiles, uint32_t *order_out,
                             uint32_t *live_out, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!stop || !order_out || !live_out) return fail(c, RT_ERR_ARG, "rt_tile_stop_order: null argument");
    if (n_tiles == 0 || n_tiles >= (1u << 28)) return fail(c, RT_ERR_ARG, "rt_tile_stop_order: n_tiles is 0 or above 2^28 - 1");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_tile_stop_order: flags other than RT_OUT_DEVICE");
    const size_t nb = (size_t)n_tiles * sizeof(uint32_t);
    if (overlaps(order_out, nb, base, nb) || overlaps(order_out, nb, stop, nb) || overlaps(order_out, nb, live_out, 4) ||
        overlaps(live_out, 4, base, nb) || overlaps(live_out, 4, stop, nb))
        return fail(c, RT_ERR_ARG, "rt_tile_stop_order: an output overlaps an input or the other output");
    AuxCall x = {c, RT_ST_STOP_ORDER};
    if (const int r = x.open(stream, flags)) return r;
    const Plane pl[] = {{reinterpret_cast<const float *>(base), nullptr, base ? n_tiles : 0u},
                        {reinterpret_cast<const float *>(stop), nullptr, n_tiles},
                        {nullptr, reinterpret_cast<float *>(order_out), n_tiles},
                        {nullptr, reinterpret_cast<float *>(live_out), 1}};
    if (const int r = x.begin(pl, 4)) return r;
    const int e = rt_launch_order_stop(base ? x.words(0, base) : nullptr, x.words(1, stop), n_tiles, x.words(2, order_out),
                                       x.words(3, live_out), x.st);
    if (e) return hip_fail(c, (hipError_t)e, "masked order kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_tile_stop_order(rt_ctx *c, const uint32_t *base, const uint32_t *stop, uint32_t n_tiles, uint32_t *order_out,
                       uint32_t *live_out, int flags)
try {
    return finish_sync(c, rt_tile_stop_order_async(c, base, stop, n_tiles, order_out, live_out, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_last_adaptive_ms(const rt_ctx *c, float *select_ms, float *order_ms)
try {
    return last_ms(c, {{RT_ST_STOP_SELECT, select_ms}, {RT_ST_STOP_ORDER, order_ms}});
} RT_CATCH(err_of(c))

/* ---- per-tile sample counts -------------------------------- */

int rt_fold_tiles_async(rt_ctx *c, const float *sample_rgba, float *acc_rgba, uint32_t *count_io, const uint32_t *passes,
                        uint32_t pass, const float *mom_in, float *mom_out, float *len_out, uint32_t W, uint32_t H, int flags,
                        void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!sample_rgba || !acc_rgba || !count_io) return fail(c, RT_ERR_ARG, "rt_fold_tiles: null argument");
    if (!mom_in != !mom_out) return fail(c, RT_ERR_ARG, "rt_fold_tiles: one of mom_in and mom_out is null");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_fold_tiles: flags other than RT_OUT_DEVICE");
    const size_t px = (size_t)W * H, tiles = (size_t)((W + 7u) / 8u) * ((H + 7u) / 8u);
    /* every buffer apart from every other; the moments may be one buffer exactly */
    const struct {
        const void *p;
        size_t bytes;
    } buf[] = {{sample_rgba, 4 * px * sizeof(float)}, {acc_rgba, 4 * px * sizeof(float)}, {count_io, tiles * sizeof(uint32_t)},
               {passes, tiles * sizeof(uint32_t)},    {len_out, px * sizeof(float)},       {mom_in, 4 * px * sizeof(float)},
               {mom_out, 4 * px * sizeof(float)}};
    for (int o = 1; o < 7; ++o)
        for (int i = 0; i < o; ++i)
            if (!(o == 6 && i == 5 && mom_in == mom_out) && overlaps(buf[o].p, buf[o].bytes, buf[i].p, buf[i].bytes))
                return fail(c, RT_ERR_ARG, "rt_fold_tiles: the buffers overlap");
    AuxCall x = {c, RT_ST_FOLD};
    if (const int r = x.open(stream, flags)) return r;
    /* staged: the sample, the accumulation buffer and the counts (both updated in place there), the passes,
       the moments (in place there: an unfolded tile keeps them), then the lengths */
    const Plane pl[] = {{sample_rgba, nullptr, 4 * px},
                        {acc_rgba, acc_rgba, 4 * px},
                        {reinterpret_cast<const float *>(count_io), reinterpret_cast<float *>(count_io), tiles},
                        {reinterpret_cast<const float *>(passes), nullptr, passes ? tiles : 0u},
                        {mom_in, mom_out, mom_in ? 4 * px : 0u},
                        {nullptr, len_out, len_out ? px : 0u}};
    if (const int r = x.begin(pl, 6)) return r;
    const int e = rt_launch_fold_tiles(x.at(0, sample_rgba), x.at(1, acc_rgba), x.words(2, count_io),
                                       passes ? x.words(3, passes) : nullptr, pass, mom_in ? x.at(4, mom_in) : nullptr,
                                       mom_out ? x.at(4, mom_out) : nullptr, len_out ? x.at(5, len_out) : nullptr, W, H, x.st);
    if (e) return hip_fail(c, (hipError_t)e, "fold kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_fold_tiles(rt_ctx *c, const float *sample_rgba, float *acc_rgba, uint32_t *count_io, const uint32_t *passes, uint32_t pass,
                  const float *mom_in, float *mom_out, float *len_out, uint32_t W, uint32_t H, int flags)
try {
    return finish_sync(c, rt_fold_tiles_async(c, sample_rgba, acc_rgba, count_io, passes, pass, mom_in, mom_out, len_out, W, H,
                                              flags, nullptr));
} RT_CATCH(err_of(c))

int rt_budget_defaults(rt_budget_params *p)
try {
    if (!p) return RT_ERR_ARG;
    p->max_passes = 4;
    float lim = 0.1f; /* rt_noise_defaults' threshold x 2, 4, 8, ... (exact doublings) */
    for (float &l : p->limits) {
        l = lim;
        lim = lim * 2.0f;
    }
    return RT_OK;
} RT_CATCH(nullptr)

int rt_tile_budget_async(rt_ctx *c, const float *tiles_mean_max, const uint32_t *stop, uint32_t *passes_out,
                         rt_budget_stats *stats_out, uint32_t W, uint32_t H, const rt_budget_params *prm, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!tiles_mean_max || !passes_out || !stats_out || !prm) return fail(c, RT_ERR_ARG, "rt_tile_budget: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_tile_budget: flags other than RT_OUT_DEVICE");
    if (prm->max_passes < 1 || prm->max_passes > RT_BUDGET_MAX_PASSES)
        return fail(c, RT_ERR_ARG, "rt_tile_budget: max_passes outside 1..8");
    for (uint32_t k = 0; k + 1 < prm->max_passes; ++k)
        if (!(prm->limits[k] >= 0.0f) || (k && !(prm->limits[k] > prm->limits[k - 1])))
            return fail(c, RT_ERR_ARG, "rt_tile_budget: a limit is NaN, negative or not above the one before it");
    const size_t tiles = (size_t)((W + 7u) / 8u) * ((H + 7u) / 8u);
    const struct {
        const void *p;
        size_t bytes;
    } buf[] = {{tiles_mean_max, 2 * tiles * sizeof(float)}, {stop, tiles * sizeof(uint32_t)},
               {passes_out, tiles * sizeof(uint32_t)},      {stats_out, sizeof(rt_budget_stats)}};
    for (int o = 2; o < 4; ++o)
        for (int i = 0; i < o; ++i)
            if (overlaps(buf[o].p, buf[o].bytes, buf[i].p, buf[i].bytes))
                return fail(c, RT_ERR_ARG, "rt_tile_budget: an output overlaps an input or the other output");
    AuxCall x = {c, RT_ST_BUDGET};
    if (const int r = x.open(stream, flags)) return r;
    constexpr size_t kStatWords = sizeof(rt_budget_stats) / sizeof(float);
    const Plane pl[] = {{tiles_mean_max, nullptr, 2 * tiles},
                        {reinterpret_cast<const float *>(stop), nullptr, stop ? tiles : 0u},
                        {nullptr, reinterpret_cast<float *>(passes_out), tiles},
                        {nullptr, reinterpret_cast<float *>(stats_out), kStatWords}};
    if (const int r = x.begin(pl, 4)) return r;
    const int e = rt_launch_tile_budget(x.at(0, tiles_mean_max), stop ? x.words(1, stop) : nullptr, x.words(2, passes_out), W, H,
                                        prm->max_passes, prm->limits, x.words(3, stats_out), x.st);
    if (e) return hip_fail(c, (hipError_t)e, "budget rule kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_tile_budget(rt_ctx *c, const float *tiles_mean_max, const uint32_t *stop, uint32_t *passes_out, rt_budget_stats *stats_out,
                   uint32_t W, uint32_t H, const rt_budget_params *prm, int flags)
try {
    return finish_sync(c, rt_tile_budget_async(c, tiles_mean_max, stop, passes_out, stats_out, W, H, prm, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_tile_pass_mask_async(rt_ctx *c, const uint32_t *stop, const uint32_t *passes, uint32_t pass, uint32_t *mask_out, uint32_t W,
                            uint32_t H, int flags, void *stream)
try {
    if (!c) return RT_ERR_ARG;
    if (!passes || !mask_out) return fail(c, RT_ERR_ARG, "rt_tile_pass_mask: null argument");
    if (!frame_ok(W, H)) return fail(c, RT_ERR_ARG, "bad frame size");
    if (flags & ~RT_OUT_DEVICE) return fail(c, RT_ERR_ARG, "rt_tile_pass_mask: flags other than RT_OUT_DEVICE");
    const size_t tiles = (size_t)((W + 7u) / 8u) * ((H + 7u) / 8u), tb = tiles * sizeof(uint32_t);
    if (overlaps(mask_out, tb, stop, tb) || overlaps(mask_out, tb, passes, tb))
        return fail(c, RT_ERR_ARG, "rt_tile_pass_mask: the output overlaps an input");
    AuxCall x = {c, RT_ST_PASS_MASK};
    if (const int r = x.open(stream, flags)) return r;
    const Plane pl[] = {{reinterpret_cast<const float *>(stop), nullptr, stop ? tiles : 0u},
                        {reinterpret_cast<const float *>(passes), nullptr, tiles},
                        {nullptr, reinterpret_cast<float *>(mask_out), tiles}};
    if (const int r = x.begin(pl, 3)) return r;
    const int e = rt_launch_pass_mask(stop ? x.words(0, stop) : nullptr, x.words(1, passes), pass, W, H, x.words(2, mask_out), x.st);
    if (e) return hip_fail(c, (hipError_t)e, "pass mask kernel launch");
    return x.end();
} RT_CATCH(err_of(c))

int rt_tile_pass_mask(rt_ctx *c, const uint32_t *stop, const uint32_t *passes, uint32_t pass, uint32_t *mask_out, uint32_t W,
                      uint32_t H, int flags)
try {
    return finish_sync(c, rt_tile_pass_mask_async(c, stop, passes, pass, mask_out, W, H, flags, nullptr));
} RT_CATCH(err_of(c))

int rt_last_budget_ms(const rt_ctx *c, float *fold_ms, float *budget_ms, float *mask_ms)
try {
    return last_ms(c, {{RT_ST_FOLD, fold_ms}, {RT_ST_BUDGET, budget_ms}, {RT_ST_PASS_MASK, mask_ms}});
} RT_CATCH(err_of(c))

} /* extern "C" */
