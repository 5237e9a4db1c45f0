/*
 * rt_render — headless C++ host over RayTracerHIP.hpp: the reference's
 * clrt/main.cpp (sphere scene) and clrt/plymain.cpp (+ a triangle mesh) without
 * the GLUT window.  Frames are driven like GlutCLWindow (progression 0, 1, 2, ...;
 * GlutCLWindow.cpp:144-158) and the last frame is written as raw RGBA32F
 * (W*H*4 little-endian floats) and/or a PFM.
 *
 *   rt_render [--scene main|ply] [--width W] [--height H] [--frames F]
 *             [--sample-rate S] [--depth D] [--mesh N_TRIS | --ply FILE] [--linear]
 *             [--raw out.f32] [--pfm out.pfm] [--device K]
 *             [--builder host|gpu|ploc]   (the mesh's BVH builder, RayTracerHIP::setBuilder; default host.
 *              Every builder gives the same frames)
 *             [--build-lights]   (with --builder gpu|ploc: RT_BUILD_OPT_LIGHTS, the never-hit triangles left
 *              out and the shadow tree split by what can occlude the lights; the same frames again)
 *             [--collapse greedy|sah]   (with --builder gpu|ploc: RT_COLLAPSE_*, how the binary tree becomes the
 *              4-wide one, RayTracerHIP::setCollapse; default greedy; the same frames again)
 *             [--events d,d,l,d,m:5:-3,s:64:32,d,...]   (interactive replay: ProgressiveViewHIP
 *              display / arrow keys l r u n / drag motion / reshape, GlutCLWindow.cpp:136-301;
 *              one JSON line per event on stdout: the view state and whether a redisplay was
 *              posted) [--max-progression N] [--frames-out FILE]   (every displayed frame,
 *              appended as raw RGBA32F)
 *             [--denoise [ITER]]   (the display denoiser, ITER passes (default 5): the frame written by
 *              --raw / --pfm stays the raw one; the filtered frame goes to --denoised FILE (raw RGBA32F)
 *              and / or --denoised-pfm FILE; with --events the view displays the filtered frame
 *              (ProgressiveViewHIP::setDenoise): --frames-out holds what it shows, --raw-frames-out FILE
 *              the accumulation buffer of every displayed frame)
 *             [--temporal [MAXHIST]]   (with --events: the view carries its displayed frame across camera
 *              moves (ProgressiveViewHIP::setTemporal, history capped at MAXHIST frames, default 32), with or
 *              without --denoise: --frames-out holds what it shows, --raw-frames-out and --features-out as above)
 *             [--variance-guided [SIGMA_LUM]]   (with --events: the view displays the variance-guided filter
 *              (ProgressiveViewHIP::setVarianceGuided, luminance tolerance SIGMA_LUM standard deviations, default 4)
 *              in place of --denoise's, with or without --temporal: --frames-out holds what it shows,
 *              --raw-frames-out and --features-out as above)
 *             [--poses FILE]   (with --events and --mesh / --ply: raw float32, K poses of 3 * n_verts floats
 *              each, of the mesh's vertices; the event p:K calls ProgressiveViewHIP::updateMesh(pose K), its
 *              JSON line names what the tracer did: "mesh_update": "refit" | "rebuilt")
 *             [--motion-carry [MAXHIST]]   (with --temporal: the view carries its displayed frame across the
 *              p events too (ProgressiveViewHIP::setMotionCarry, that carry's history capped at MAXHIST frames,
 *              default 8))
 *             [--history-trust [TOL]]   (with --temporal: the view judges its carried history at every display
 *              (ProgressiveViewHIP::setHistoryTrust, tolerance TOL standard deviations, default rt_trust_defaults';
 *              "inf" trusts everything); the event e:DX:DY:DZ moves every emissive sphere by (DX, DY, DZ) and
 *              calls ProgressiveViewHIP::sceneChanged())
 *             [--sphere-carry [MAXHIST]]   (with --temporal: the view carries its displayed frame across the
 *              o events (ProgressiveViewHIP::setSphereCarry, that carry's history capped at MAXHIST frames,
 *              default 8); the event o:I:DX:DY:DZ[:DR] adds (DX, DY, DZ) to the centre of sphere I of the scene
 *              and DR to its radius (cumulative, like e), rebuilds the scene in the same order and calls
 *              ProgressiveViewHIP::sceneChanged())
 *             [--tonemap [clamp|reinhard|aces]]   (the tone-mapped 8-bit display output, default aces
 *              (rt_tonemap; with --events ProgressiveViewHIP::setToneMap: the float frames of --frames-out stay what
 *              they are without it) [--exposure auto|VALUE] (the histogram meter, the default, or a fixed factor)
 *              [--adapt RATE] (the meter's rate, default 1) [--no-srgb] [--no-dither]
 *              [--ppm FILE] (binary P6 of the final shown 8-bit frame, top row first: flipped like the PFM)
 *              [--frames8-out FILE] (with --events: every displayed RGBA8 frame, appended as W*H words)
 *              [--exposure-log FILE] (with --events: per displayed frame the bits of its exposure, one hex word a line))
 *             [--converge [THRESHOLD]]   (with --events: the view refines until converged
 *              (ProgressiveViewHIP::setConverge: the noise meter's level at or under THRESHOLD, default
 *              rt_noise_defaults'); the event lines gain "converged") [--converge-percentile Q] [--converge-min-frames N]
 *              [--noise-log FILE] (per traced display one line: the level's bits in hex, counted, skipped, below,
 *              converged 0 / 1) [--noise-map-out FILE] (the tile planes of the traced displays, appended as float pairs)
 *             [--adaptive [THRESHOLD]]   (with --converge and --mesh / --ply, without --temporal: the view stops tracing
 *              the 8x8 tiles the noise meter calls quiet (ProgressiveViewHIP::setAdaptive: a tile's mean error at or
 *              under THRESHOLD, default rt_adaptive_defaults'); the event lines gain "tiles_active")
 *              [--adaptive-max-ratio R] [--adaptive-min-frames N] [--adaptive-dilate D]
 *              [--stop-map-out FILE] (the stop planes after the traced displays, appended as words)
 *             [--budget [MAXPASSES]]   (with --adaptive: the noisy tiles get up to MAXPASSES passes per display
 *              (ProgressiveViewHIP::setSampleBudget, default rt_budget_defaults'); the event lines gain "rounds" and
 *              "tile_passes") [--budget-limits A,B,...] (the mean errors above which a tile gets one more pass each)
 *              [--budget-log FILE] (per traced display one line: rounds, tile_passes, then the tiles with 0, 1, ... 8
 *              passes, as the budget rule left them for the next display) [--counts-out FILE] (the count planes
 *              after the traced displays, appended as words)
 *             [--adaptive-history]   (with --adaptive and --temporal, which are refused together without it: the tiles
 *              stop by the length of their merged history (ProgressiveViewHIP::setAdaptiveHistory); --stop-map-out,
 *              --counts-out, --noise-log, --budget-log and "tiles_active" as under --adaptive)
 *              [--history-len-out FILE] (with --temporal: the kept history lengths after the traced displays, appended
 *              as W*H floats)
 *             [--features-out FILE]   (the first-hit feature buffer, 2 planes of W*H float4, of the last
 *              frame; with --events appended for every displayed frame)
 *             [--tile STRIPE,N,R]   (this process renders rank R's row stripes of N: the raw output
 *              is the compact tile — the sharding path rehearsed as separate processes)
 *             [--comm-ranks N --comm-rank R --comm-id FILE]   (native multi-GPU: one process per
 *              GPU, librtmi's RCCL communicator; rank 0 writes the id to FILE, the others read
 *              it; rt_comm_render per frame, the assembled frame written by rank 0)
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <fstream>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ProgressiveViewHIP.hpp"
#include "RayTracerHIP.hpp"

namespace {

/* init_material / init_sphere, clrt/main.cpp:13-42 */
rt_sphere init_sphere()
{
    rt_sphere s;
    std::memset(&s, 0, sizeof(s));
    s.radius = 1.0f;
    s.mat.specExp = 1000000.0f;
    s.mat.ior = 1.0f;
    s.mat.refExp = 1000000.0f;
    return s;
}

constexpr unsigned kSceneSpheres = 6; /* of add_scene */
/* the o events so far, per sphere: what is added to its centre and to its radius */
using SphereOffsets = std::array<std::array<float, 4>, kSceneSpheres>;

/* clrt/main.cpp:44-110 (ply = clrt/plymain.cpp:45-111) */
void add_scene(RayTracerHIP &rt, bool ply, rt_vec3 light_offset = {0.0f, 0.0f, 0.0f}, const SphereOffsets *moved = nullptr)
{
    /* the scene's spheres in order, each moved by its o events (an untouched sphere keeps its bits) */
    unsigned n = 0;
    const auto add = [&](rt_sphere s) {
        const std::array<float, 4> o = moved ? (*moved)[n] : std::array<float, 4>{};
        if (o[0] != 0.0f || o[1] != 0.0f || o[2] != 0.0f || o[3] != 0.0f) {
            s.center = {s.center.x + o[0], s.center.y + o[1], s.center.z + o[2]};
            s.radius += o[3];
        }
        ++n;
        rt.addSphere(s);
    };
    rt_sphere s = init_sphere();
    s.center = {-2.0f, -4.0f, -2.0f};
    s.mat.kd = 1.0f;
    s.mat.diffuse = {0.0f, 0.7f, 0.7f};
    add(s);
    s = init_sphere();
    s.center = {2.0f, -3.0f, 2.0f};
    s.mat.ks = 0.2f;
    s.mat.kt = 0.8f;
    s.mat.extinction = ply ? rt_vec3{0.95f, 0.85f, 0.90f} : rt_vec3{0.99f, 0.95f, 0.95f};
    s.mat.ior = 1.1f;
    add(s);
    s = init_sphere();
    s.center = {0.0f, -4.0f, 0.0f};
    s.mat.ks = 1.0f;
    add(s);
    s = init_sphere();
    s.center = {2.0f, -4.0f, -2.0f};
    s.mat.kd = 0.2f;
    s.mat.ks = 0.8f;
    s.mat.diffuse = {0.7f, 0.7f, 0.0f};
    s.mat.specExp = 100.0f;
    add(s);
    s = init_sphere();
    s.center = {-2.0f, -4.0f, 2.0f};
    s.mat.kd = 0.6f;
    s.mat.ks = 0.4f;
    s.mat.diffuse = {0.7f, 0.0f, 0.8f};
    s.mat.specExp = 1000.0f;
    add(s);
    s = init_sphere();
    s.center = ply ? rt_vec3{0.0f, 4.0f, 2.0f} : rt_vec3{2.2f, 1.0f, 2.0f};
    s.center = {s.center.x + light_offset.x, s.center.y + light_offset.y, s.center.z + light_offset.z}; /* (the e event) */
    s.radius = 0.5f;
    s.mat.emission_power = 1.0f;
    const float e = ply ? 1.1f : 1.8f;
    s.mat.emission = {e, e, e};
    add(s);
}

int usage()
{
    std::fprintf(stderr, "usage: rt_render [--scene main|ply] [--width W] [--height H] [--frames F] "
                         "[--sample-rate S] [--depth D] [--mesh N | --ply FILE] [--linear] [--builder host|gpu|ploc] [--build-lights] [--collapse greedy|sah] [--raw f] [--pfm f] "
                         "[--device K] [--denoise [ITER]] [--temporal [MAXHIST]] [--variance-guided [SIGMA_LUM]] [--poses f] [--motion-carry [MAXHIST]] [--history-trust [TOL]] [--sphere-carry [MAXHIST]] (--events o:I:DX:DY:DZ[:DR] moves sphere I) [--denoised f] [--denoised-pfm f] [--features-out f] "
                         "[--raw-frames-out f] [--tonemap [clamp|reinhard|aces]] [--exposure auto|VALUE] [--adapt RATE] [--no-srgb] [--no-dither] "
                         "[--ppm f] [--frames8-out f] [--exposure-log f] [--converge [THRESHOLD]] [--converge-percentile Q] [--converge-min-frames N] "
                         "[--noise-log f] [--noise-map-out f] [--adaptive [THRESHOLD]] [--adaptive-max-ratio R] [--adaptive-min-frames N] "
                         "[--adaptive-dilate D] [--stop-map-out f] [--budget [MAXPASSES]] [--budget-limits a,b,...] [--budget-log f] [--counts-out f] [--adaptive-history] [--history-len-out f] [--tile STRIPE,N,R] [--comm-ranks N --comm-rank R --comm-id FILE]\n");
    return 2;
}

/* The communicator id travels through a file: rank 0 writes it (rename makes it appear
   whole), the other ranks wait for it. */
bool share_comm_id(const std::string &path, int rank, uint8_t id[RT_COMM_ID_BYTES])
{
    if (rank == 0) {
        if (rt_comm_get_unique_id(id) != RT_OK) return false;
        const std::string tmp = path + ".tmp";
        FILE *f = std::fopen(tmp.c_str(), "wb");
        if (!f || std::fwrite(id, 1, RT_COMM_ID_BYTES, f) != RT_COMM_ID_BYTES) return false;
        std::fclose(f);
        return std::rename(tmp.c_str(), path.c_str()) == 0;
    }
    for (int i = 0; i < 600; ++i) {
        if (FILE *f = std::fopen(path.c_str(), "rb")) {
            const size_t n = std::fread(id, 1, RT_COMM_ID_BYTES, f);
            std::fclose(f);
            if (n == RT_COMM_ID_BYTES) return true;
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
    }
    return false;
}

/* The numeric value that may follow a flag: argv[i + 1] if it starts with a digit (or, where the flag
   takes it, is "inf"), and then i moves on to it; else nullptr and the flag keeps its default. */
const char *optional_number(int argc, char **argv, int &i, bool or_inf = false)
{
    if (i + 1 >= argc) return nullptr;
    const char *v = argv[i + 1];
    const bool number = (v[0] >= '0' && v[0] <= '9') || (or_inf && !std::strcmp(v, "inf"));
    return number ? argv[++i] : nullptr;
}

/* one more frame at the end of a --frames-out / --raw-frames-out / --features-out file */
bool append(FILE *f, const std::vector<float> &frame) { return std::fwrite(frame.data(), 4, frame.size(), f) == frame.size(); }

/* binary P6 of an RGBA8 frame (bottom row first in memory), top row first */
bool write_ppm(const std::string &path, const std::vector<uint32_t> &px, unsigned W, unsigned H)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "P6\n%u %u\n255\n", W, H);
    bool ok = true;
    for (int y = (int)H - 1; y >= 0; --y)
        for (unsigned x = 0; x < W; ++x) {
            const uint32_t w = px[(size_t)y * W + x];
            const unsigned char rgb[3] = {(unsigned char)(w & 255u), (unsigned char)(w >> 8 & 255u), (unsigned char)(w >> 16 & 255u)};
            ok = ok && std::fwrite(rgb, 1, 3, f) == 3;
        }
    return std::fclose(f) == 0 && ok;
}

} // namespace

int main(int argc, char **argv)
{
    std::string scene = "main", raw, pfm, ply_path, events, comm_id, frames_out, den_raw, den_pfm, feat_out, raw_frames_out, poses_path;
    bool denoise = false, temporal = false, var_guided = false, motion_carry = false, trust = false, sphere_carry = false;
    float sphere_max_history = 8.0f;
    std::string ppm, frames8_out, exposure_log;
    bool tonemap = false, auto_exposure = true;
    rt_tonemap_params tone_params = RayTracerHIP::toneMapDefaults();
    rt_meter_params meter_params = RayTracerHIP::meterDefaults();
    rt_trust_params trust_params = RayTracerHIP::trustDefaults();
    bool converge = false;
    rt_noise_params noise_params = RayTracerHIP::noiseDefaults();
    unsigned converge_min_frames = 8;
    std::string noise_log, noise_map_out;
    bool adaptive = false;
    rt_adaptive_params adaptive_params = RayTracerHIP::adaptiveDefaults();
    std::string stop_map_out;
    bool budget = false;
    rt_budget_params budget_params = RayTracerHIP::budgetDefaults();
    std::string budget_log, counts_out;
    bool adaptive_history = false;
    std::string history_len_out;
    float motion_max_history = 8.0f;
    rt_denoise_var_params var_params = RayTracerHIP::denoiseVarDefaults();
    rt_reproject_params temporal_params = RayTracerHIP::reprojectDefaults();
    rt_denoise_params den_params = RayTracerHIP::denoiseDefaults();
    unsigned W = 512, H = 512, frames = 1, sr = 1, depth = 6, n_tris = 0, max_prog = 10000;
    int device = 0, comm_ranks = 0, comm_rank = 0;
    rt_tile tile{8, 1, 0};
    bool linear = false;
    int builder = RT_BUILD_HOST;
    bool build_lights = false;
    int collapse = RT_COLLAPSE_GREEDY;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char * { return i + 1 < argc ? argv[++i] : nullptr; };
        const char *v = nullptr;
        if (a == "--linear") {
            linear = true;
            continue;
        }
        if (a == "--build-lights") {
            build_lights = true;
            continue;
        }
        if (a == "--adaptive-history") {
            adaptive_history = true;
            continue;
        }
        if (a == "--no-srgb" || a == "--no-dither") {
            (a == "--no-srgb" ? tone_params.srgb : tone_params.dither) = 0;
            continue;
        }
        if (a == "--tonemap") { /* an optional curve follows */
            tonemap = true;
            const char *names[] = {"clamp", "reinhard", "aces"};
            for (unsigned k = 0; k < 3 && i + 1 < argc; ++k)
                if (!std::strcmp(argv[i + 1], names[k])) {
                    tone_params.curve = k;
                    ++i;
                    break;
                }
            continue;
        }
        if (a == "--denoise") { /* an optional pass count follows */
            denoise = true;
            if ((v = optional_number(argc, argv, i))) den_params.iterations = (unsigned)std::atoi(v);
            continue;
        }
        if (a == "--temporal") { /* an optional history cap follows */
            temporal = true;
            if ((v = optional_number(argc, argv, i))) temporal_params.max_history = (float)std::atof(v);
            continue;
        }
        if (a == "--motion-carry") { /* an optional history cap follows */
            motion_carry = true;
            if ((v = optional_number(argc, argv, i))) motion_max_history = (float)std::atof(v);
            continue;
        }
        if (a == "--sphere-carry") { /* an optional history cap follows */
            sphere_carry = true;
            if ((v = optional_number(argc, argv, i))) sphere_max_history = (float)std::atof(v);
            continue;
        }
        if (a == "--history-trust") { /* an optional tolerance follows ("inf": everything is trusted) */
            trust = true;
            if ((v = optional_number(argc, argv, i, true))) trust_params.tolerance = (float)std::atof(v);
            continue;
        }
        if (a == "--variance-guided") { /* an optional luminance tolerance follows */
            var_guided = true;
            if ((v = optional_number(argc, argv, i))) var_params.sigma_lum = (float)std::atof(v);
            continue;
        }
        if (a == "--converge") { /* an optional threshold follows */
            converge = true;
            if ((v = optional_number(argc, argv, i))) noise_params.threshold = (float)std::atof(v);
            continue;
        }
        if (a == "--adaptive") { /* an optional threshold follows */
            adaptive = true;
            if ((v = optional_number(argc, argv, i))) adaptive_params.threshold = (float)std::atof(v);
            continue;
        }
        if (a == "--budget") { /* an optional pass count follows */
            budget = true;
            if ((v = optional_number(argc, argv, i))) budget_params.max_passes = (unsigned)std::atoi(v);
            continue;
        }
        if (!(v = next())) return usage();
        if (a == "--scene") scene = v;
        else if (a == "--budget-limits") { /* (the library checks them) */
            int k = 0;
            for (const char *q = v; *q && k < RT_BUDGET_MAX_PASSES - 1; ++k) {
                char *end = nullptr;
                budget_params.limits[k] = std::strtof(q, &end);
                if (end == q) return usage();
                q = *end == ',' ? end + 1 : end;
            }
        }
        else if (a == "--budget-log") budget_log = v;
        else if (a == "--counts-out") counts_out = v;
        else if (a == "--history-len-out") history_len_out = v;
        else if (a == "--adaptive-max-ratio") adaptive_params.max_ratio = (float)std::atof(v); /* ("inf": the term is off) */
        else if (a == "--adaptive-min-frames") adaptive_params.min_frames = (unsigned)std::atoi(v);
        else if (a == "--adaptive-dilate") adaptive_params.dilate = (unsigned)std::atoi(v);
        else if (a == "--stop-map-out") stop_map_out = v;
        else if (a == "--converge-percentile") noise_params.percentile = (float)std::atof(v);
        else if (a == "--converge-min-frames") converge_min_frames = (unsigned)std::atoi(v);
        else if (a == "--noise-log") noise_log = v;
        else if (a == "--noise-map-out") noise_map_out = v;
        else if (a == "--denoised") den_raw = v;
        else if (a == "--denoised-pfm") den_pfm = v;
        else if (a == "--features-out") feat_out = v;
        else if (a == "--raw-frames-out") raw_frames_out = v;
        else if (a == "--ppm") ppm = v;
        else if (a == "--frames8-out") frames8_out = v;
        else if (a == "--exposure-log") exposure_log = v;
        else if (a == "--adapt") meter_params.rate = (float)std::atof(v);
        else if (a == "--exposure") {
            auto_exposure = !std::strcmp(v, "auto");
            if (!auto_exposure) tone_params.exposure = (float)std::atof(v);
        }
        else if (a == "--width") W = (unsigned)std::atoi(v);
        else if (a == "--height") H = (unsigned)std::atoi(v);
        else if (a == "--frames") frames = (unsigned)std::atoi(v);
        else if (a == "--sample-rate") sr = (unsigned)std::atoi(v);
        else if (a == "--depth") depth = (unsigned)std::atoi(v);
        else if (a == "--mesh") n_tris = (unsigned)std::atoi(v);
        else if (a == "--ply") ply_path = v;
        else if (a == "--collapse") {
            if (!std::strcmp(v, "greedy")) collapse = RT_COLLAPSE_GREEDY;
            else if (!std::strcmp(v, "sah")) collapse = RT_COLLAPSE_SAH;
            else return usage();
        }
        else if (a == "--builder") {
            if (!std::strcmp(v, "host")) builder = RT_BUILD_HOST;
            else if (!std::strcmp(v, "gpu")) builder = RT_BUILD_GPU;
            else if (!std::strcmp(v, "ploc")) builder = RT_BUILD_GPU_PLOC;
            else return usage();
        }
        else if (a == "--events") events = v;
        else if (a == "--poses") poses_path = v;
        else if (a == "--max-progression") max_prog = (unsigned)std::atoi(v);
        else if (a == "--frames-out") frames_out = v;
        else if (a == "--raw") raw = v;
        else if (a == "--pfm") pfm = v;
        else if (a == "--device") device = std::atoi(v);
        else if (a == "--tile") {
            if (std::sscanf(v, "%u,%u,%u", &tile.stripe_rows, &tile.n_ranks, &tile.rank) != 3) return usage();
        } else if (a == "--comm-ranks") comm_ranks = std::atoi(v);
        else if (a == "--comm-rank") comm_rank = std::atoi(v);
        else if (a == "--comm-id") comm_id = v;
        else return usage();
    }
    const bool ply = scene == "ply" || n_tris > 0 || !ply_path.empty();
    if (temporal && events.empty()) {
        std::fprintf(stderr, "rt_render: --temporal needs --events (it carries the display across camera moves)\n");
        return 2;
    }
    if (motion_carry && !temporal) {
        std::fprintf(stderr, "rt_render: --motion-carry needs --temporal (without it there is nothing to carry)\n");
        return 2;
    }
    if (sphere_carry && !temporal) {
        std::fprintf(stderr, "rt_render: --sphere-carry needs --temporal (without it there is nothing to carry)\n");
        return 2;
    }
    for (size_t pos = 0; pos <= events.size();) { /* the o events name spheres of the scene */
        const size_t end = std::min(events.find(',', pos), events.size());
        const std::string ev = events.substr(pos, end - pos);
        pos = end + 1;
        unsigned k = 0;
        if (ev.empty() || ev[0] != 'o') continue;
        if (std::sscanf(ev.c_str() + 1, ":%u", &k) != 1 || ev[2] == '-') return usage();
        if (k >= kSceneSpheres) {
            std::fprintf(stderr, "rt_render: event %s: the scene holds no sphere %u (it has %u)\n", ev.c_str(), k, kSceneSpheres);
            return 2;
        }
    }
    if (trust && !temporal) {
        std::fprintf(stderr, "rt_render: --history-trust needs --temporal (without it there is no history to judge)\n");
        return 2;
    }
    if (!tonemap && (!ppm.empty() || !frames8_out.empty() || !exposure_log.empty())) {
        std::fprintf(stderr, "rt_render: --ppm / --frames8-out / --exposure-log need --tonemap (there is no 8-bit frame without it)\n");
        return 2;
    }
    if (events.empty() && (!frames8_out.empty() || !exposure_log.empty())) {
        std::fprintf(stderr, "rt_render: --frames8-out / --exposure-log need --events (they follow a view's displays)\n");
        return 2;
    }
    if (var_guided && events.empty()) {
        std::fprintf(stderr, "rt_render: --variance-guided needs --events (it follows a view's progressive frames)\n");
        return 2;
    }
    if (converge && events.empty()) {
        std::fprintf(stderr, "rt_render: --converge needs --events (it follows a view's progressive frames)\n");
        return 2;
    }
    if (!converge && (!noise_log.empty() || !noise_map_out.empty())) {
        std::fprintf(stderr, "rt_render: --noise-log / --noise-map-out need --converge (nothing is metered without it)\n");
        return 2;
    }
    if (adaptive && !converge) {
        std::fprintf(stderr, "rt_render: --adaptive needs --converge (it stops tiles by the noise meter's map)\n");
        return 2;
    }
    if (adaptive_history && !adaptive) {
        std::fprintf(stderr, "rt_render: --adaptive-history needs --adaptive (it lets the stop rule run under --temporal)\n");
        return 2;
    }
    if (adaptive_history && !temporal) {
        std::fprintf(stderr, "rt_render: --adaptive-history needs --temporal (the tiles stop by their merged history)\n");
        return 2;
    }
    if (!history_len_out.empty() && !temporal) {
        std::fprintf(stderr, "rt_render: --history-len-out needs --temporal (there is no history without it)\n");
        return 2;
    }
    if (adaptive && temporal && !adaptive_history) {
        std::fprintf(stderr, "rt_render: --adaptive does not go with --temporal (the merged history has no per-tile frame count)\n");
        return 2;
    }
    if (adaptive && n_tris == 0 && ply_path.empty()) {
        std::fprintf(stderr, "rt_render: --adaptive needs --mesh or --ply (the sphere kernels' seed rows shift with the progression)\n");
        return 2;
    }
    if (budget && !adaptive) {
        std::fprintf(stderr, "rt_render: --budget needs --adaptive (the passes go to the tiles it leaves live)\n");
        return 2;
    }
    if (!budget && (!budget_log.empty() || !counts_out.empty())) {
        std::fprintf(stderr, "rt_render: --budget-log / --counts-out need --budget (there is no count plane without it)\n");
        return 2;
    }
    if (!adaptive && !stop_map_out.empty()) {
        std::fprintf(stderr, "rt_render: --stop-map-out needs --adaptive (there is no stop plane without it)\n");
        return 2;
    }
    try {
        RayTracerHIP rt(device);
        add_scene(rt, ply);
        rt.setSampleRate(sr);
        rt.setMaxPathDepth(depth);
        const float target[3] = {0.0f, -4.0f, 0.0f};
        if (ply) rt.setCameraSpherical(target, 40.0f, 105.0f, 5.0f); /* plymain.cpp:115-117 */
        else rt.setCameraSpherical(target, 14.0f, 118.0f, 5.0f);     /* main.cpp:127-128 */
        int kernel = RT_KERNEL_SPHERES;
        rt.setBuilder(builder);
        rt.setBuildOptions(build_lights ? RT_BUILD_OPT_LIGHTS : 0u);
        rt.setCollapse(collapse);
        uint32_t n_verts = 0; /* of the mesh (--poses) */
        if (!ply_path.empty()) { /* plymain.cpp:121, with the mesh actually handed to the tracer */
            rt.setMeshFromPly(ply_path.c_str());
            rt_ply *hdr = nullptr;
            uint32_t nt = 0;
            if (rt_ply_open(ply_path.c_str(), &hdr, &n_verts, &nt) == RT_OK) rt_ply_close(hdr);
            rt.setTraversal(linear ? RT_TRAVERSAL_LINEAR : RT_TRAVERSAL_BVH);
            kernel = RT_KERNEL_TRIS;
        } else if (n_tris) {
            std::vector<float> v(3ull * rt_mesh_vertex_count(n_tris));
            std::vector<int> idx(3ull * n_tris);
            if (rt_make_mesh(n_tris, 0.0f, -2.2f, 0.0f, 2.5f, v.data(), idx.data()) != RT_OK) return 1;
            rt.setMesh(v.data(), (unsigned)(v.size() / 3), idx.data(), n_tris);
            n_verts = (uint32_t)(v.size() / 3);
            rt.setTraversal(linear ? RT_TRAVERSAL_LINEAR : RT_TRAVERSAL_BVH);
            kernel = RT_KERNEL_TRIS;
        }
        if (!events.empty()) { /* interactive replay through the display state machine */
            ProgressiveViewHIP view(rt, W, H, kernel);
            view.setProgressive(max_prog);
            if (denoise) view.setDenoise(true, den_params);
            if (temporal) view.setTemporal(true, temporal_params);
            if (var_guided) view.setVarianceGuided(true, var_params);
            if (motion_carry) view.setMotionCarry(true, motion_max_history);
            if (trust) view.setHistoryTrust(true, trust_params);
            if (sphere_carry) view.setSphereCarry(true, sphere_max_history);
            if (tonemap) view.setToneMap(true, tone_params, auto_exposure, meter_params);
            if (converge) view.setConverge(true, noise_params, converge_min_frames);
            if (!noise_map_out.empty()) view.setNoiseMapReadback(true);
            if (adaptive) view.setAdaptive(true, adaptive_params);
            if (!stop_map_out.empty()) view.setStopMapReadback(true);
            if (adaptive_history) view.setAdaptiveHistory(true);
            if (!history_len_out.empty()) view.setHistoryLengthReadback(true);
            if (budget) view.setSampleBudget(true, budget_params);
            if (!counts_out.empty()) view.setSampleCountReadback(true);
            rt_vec3 light_offset = {0.0f, 0.0f, 0.0f}; /* the e events so far */
            SphereOffsets sphere_offsets{};            /* the o events so far */
            std::vector<float> poses; /* --poses: K poses of 3 n_verts floats */
            if (!poses_path.empty()) {
                std::ifstream pf(poses_path, std::ios::binary | std::ios::ate);
                const std::streamoff bytes = pf ? (std::streamoff)pf.tellg() : -1;
                if (!n_verts || bytes <= 0 || bytes % (12 * (std::streamoff)n_verts)) {
                    std::fprintf(stderr, "rt_render: --poses needs a mesh and a file of whole poses (3 * %u floats each)\n", n_verts);
                    return 2;
                }
                poses.resize((size_t)bytes / 4);
                pf.seekg(0);
                if (!pf.read(reinterpret_cast<char *>(poses.data()), bytes)) return 1;
            }
            FILE *fo = frames_out.empty() ? nullptr : std::fopen(frames_out.c_str(), "wb");
            if (!frames_out.empty() && !fo) return 1;
            FILE *fr = raw_frames_out.empty() ? nullptr : std::fopen(raw_frames_out.c_str(), "wb");
            FILE *ff = feat_out.empty() ? nullptr : std::fopen(feat_out.c_str(), "wb");
            if ((!raw_frames_out.empty() && !fr) || (!feat_out.empty() && !ff)) return 1;
            FILE *f8 = frames8_out.empty() ? nullptr : std::fopen(frames8_out.c_str(), "wb");
            FILE *fe = exposure_log.empty() ? nullptr : std::fopen(exposure_log.c_str(), "w");
            if ((!frames8_out.empty() && !f8) || (!exposure_log.empty() && !fe)) return 1;
            FILE *fn = noise_log.empty() ? nullptr : std::fopen(noise_log.c_str(), "w");
            FILE *fm = noise_map_out.empty() ? nullptr : std::fopen(noise_map_out.c_str(), "wb");
            if ((!noise_log.empty() && !fn) || (!noise_map_out.empty() && !fm)) return 1;
            FILE *fs = stop_map_out.empty() ? nullptr : std::fopen(stop_map_out.c_str(), "wb");
            if (!stop_map_out.empty() && !fs) return 1;
            FILE *fb = budget_log.empty() ? nullptr : std::fopen(budget_log.c_str(), "w");
            FILE *fc = counts_out.empty() ? nullptr : std::fopen(counts_out.c_str(), "wb");
            if ((!budget_log.empty() && !fb) || (!counts_out.empty() && !fc)) return 1;
            FILE *fl = history_len_out.empty() ? nullptr : std::fopen(history_len_out.c_str(), "wb");
            if (!history_len_out.empty() && !fl) return 1;
            size_t pos = 0;
            while (pos <= events.size()) {
                const size_t end = std::min(events.find(',', pos), events.size());
                const std::string ev = events.substr(pos, end - pos);
                pos = end + 1;
                if (ev.empty()) continue;
                bool post = false, traced = false;
                const char *mesh_update = nullptr; /* a p event: what the tracer did */
                if (ev == "d") {
                    post = view.display();
                    traced = view.rendered();
                    if (traced && fo && !append(fo, view.pixels())) return 1;
                    if (traced && fr && !append(fr, view.rawPixels())) return 1;
                    if (traced && f8 && std::fwrite(view.pixels8().data(), 4, view.pixels8().size(), f8) != view.pixels8().size()) return 1;
                    if (traced && fe) {
                        const float e = view.exposure();
                        uint32_t u;
                        std::memcpy(&u, &e, 4);
                        std::fprintf(fe, "%08x\n", u);
                    }
                    if (traced && fn) {
                        const rt_noise_stats &ns = view.noiseStats();
                        uint32_t u;
                        std::memcpy(&u, &ns.level, 4);
                        std::fprintf(fn, "%08x %u %u %u %d\n", u, ns.counted, ns.skipped, ns.below, view.converged() ? 1 : 0);
                    }
                    if (traced && fm && !append(fm, view.noiseMap())) return 1;
                    if (traced && fs && std::fwrite(view.stopMap().data(), 4, view.stopMap().size(), fs) != view.stopMap().size()) return 1;
                    if (traced && fb) {
                        const rt_budget_stats &bs = view.budgetStats();
                        std::fprintf(fb, "%u %u", bs.rounds, bs.tile_passes);
                        for (uint32_t n : bs.by_passes) std::fprintf(fb, " %u", n);
                        std::fprintf(fb, "\n");
                    }
                    if (traced && fc && std::fwrite(view.sampleCounts().data(), 4, view.sampleCounts().size(), fc) != view.sampleCounts().size()) return 1;
                    if (traced && fl && !append(fl, view.historyLengths())) return 1;
                    if (traced && ff) {
                        std::vector<float> ft((size_t)view.width() * view.height() * 8);
                        rt.renderFeatures(ft.data(), view.width(), view.height(), kernel);
                        if (!append(ff, ft)) return 1;
                    }
                } else if (ev == "l") post = view.specialKey(ProgressiveViewHIP::KEY_LEFT);
                else if (ev == "r") post = view.specialKey(ProgressiveViewHIP::KEY_RIGHT);
                else if (ev == "u") post = view.specialKey(ProgressiveViewHIP::KEY_UP);
                else if (ev == "n") post = view.specialKey(ProgressiveViewHIP::KEY_DOWN);
                else if (ev[0] == 'm' || ev[0] == 's') {
                    int a1 = 0, a2 = 0;
                    if (std::sscanf(ev.c_str() + 1, ":%d:%d", &a1, &a2) != 2) return usage();
                    if (ev[0] == 'm') post = view.motion(a1, a2);
                    else view.reshape((unsigned)a1, (unsigned)a2);
                } else if (ev[0] == 'e') {
                    float dx = 0.0f, dy = 0.0f, dz = 0.0f;
                    if (std::sscanf(ev.c_str() + 1, ":%f:%f:%f", &dx, &dy, &dz) != 3) return usage();
                    light_offset = {light_offset.x + dx, light_offset.y + dy, light_offset.z + dz};
                    rt.clearSpheres();
                    add_scene(rt, ply, light_offset, &sphere_offsets);
                    post = view.sceneChanged();
                } else if (ev[0] == 'o') { /* (its index was checked with the arguments) */
                    unsigned k = 0;
                    float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (std::sscanf(ev.c_str() + 1, ":%u:%f:%f:%f:%f", &k, &d[0], &d[1], &d[2], &d[3]) < 4) return usage();
                    for (int j = 0; j < 4; ++j) sphere_offsets[k][j] += d[j];
                    rt.clearSpheres();
                    add_scene(rt, ply, light_offset, &sphere_offsets);
                    post = view.sceneChanged();
                } else if (ev[0] == 'p') {
                    unsigned k = 0;
                    if (std::sscanf(ev.c_str() + 1, ":%u", &k) != 1) return usage();
                    if (!n_verts || (size_t)(k + 1ull) * 3 * n_verts > poses.size()) {
                        std::fprintf(stderr, "rt_render: event %s: --poses holds no pose %u\n", ev.c_str(), k);
                        return 2;
                    }
                    post = view.updateMesh(poses.data() + (size_t)k * 3 * n_verts, n_verts);
                    mesh_update = rt.lastMeshUpdate().action == RT_MESH_UPDATE_REFIT ? "refit" : "rebuilt";
                } else return usage();
                std::printf("{\"event\": \"%s\", \"rendered\": %s, \"redisplay\": %s, \"progression\": %u, "
                            "\"azimuth\": %.9g, \"elevation\": %.9g, \"width\": %u, \"height\": %u",
                            ev.c_str(), traced ? "true" : "false", post ? "true" : "false", view.progression(),
                            view.azimuth(), view.elevation(), view.width(), view.height());
                if (mesh_update) std::printf(", \"mesh_update\": \"%s\"", mesh_update);
                if (converge) std::printf(", \"converged\": %s", view.converged() ? "true" : "false");
                if (adaptive) std::printf(", \"tiles_active\": %u", view.adaptiveStats().active);
                if (budget) std::printf(", \"rounds\": %u, \"tile_passes\": %u", view.budgetStats().rounds, view.budgetStats().tile_passes);
                std::printf("}\n");
            }
            if (fo) std::fclose(fo);
            if (fr) std::fclose(fr);
            if (ff) std::fclose(ff);
            if (f8) std::fclose(f8);
            if (fe) std::fclose(fe);
            if (fn) std::fclose(fn);
            if (fm) std::fclose(fm);
            if (fs) std::fclose(fs);
            if (fb) std::fclose(fb);
            if (fc) std::fclose(fc);
            if (fl) std::fclose(fl);
            if (!ppm.empty() && (view.pixels8().empty() || !write_ppm(ppm, view.pixels8(), view.width(), view.height()))) return 1;
            std::printf("{\"progression\": %u, \"azimuth\": %.9g, \"elevation\": %.9g, \"width\": %u, "
                        "\"height\": %u}\n",
                        view.progression(), view.azimuth(), view.elevation(), view.width(), view.height());
            if (!raw.empty()) {
                FILE *f = std::fopen(raw.c_str(), "wb");
                const std::vector<float> &px = view.pixels();
                if (!f || std::fwrite(px.data(), 4, px.size(), f) != px.size()) return 1;
                std::fclose(f);
            }
            return 0;
        }
        rt_comm *comm = nullptr;
        if (comm_ranks > 0) { /* native multi-GPU: librtmi's RCCL communicator */
            uint8_t id[RT_COMM_ID_BYTES];
            if (comm_id.empty() || !share_comm_id(comm_id, comm_rank, id)) {
                std::fprintf(stderr, "rt_render: no communicator id (--comm-id)\n");
                return 1;
            }
            if (rt_comm_create(id, comm_ranks, comm_rank, device, &comm) != RT_OK) {
                std::fprintf(stderr, "rt_render: rt_comm_create failed\n");
                return 1;
            }
        }
        const bool tiled = !comm && tile.n_ranks > 1;
        const unsigned rows = tiled ? rt_tile_rows(H, &tile) : H;
        float *dbuf = nullptr;
        if (hipMalloc(&dbuf, (size_t)W * std::max(rows, 1u) * 16) != hipSuccess) return 1;
        double rays = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned p = 0; p < frames; ++p) {
            if (comm) {
                rt.flushScene();
                if (rt_comm_render(comm, rt.handle(), dbuf, W, H, p, kernel, 8, 0) != RT_OK) {
                    std::fprintf(stderr, "rt_render: rt_comm_render: %s\n", rt_comm_last_error(comm));
                    return 1;
                }
            } else {
                rt.rayTrace(dbuf, W, H, p, kernel, true, tiled ? &tile : nullptr);
            }
            const rt_counters c = rt.counters();
            rays += (double)(c.rays_closest + c.rays_shadow);
        }
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (comm) rt_comm_destroy(comm);
        if (comm && comm_rank != 0) { /* the frame lives on rank 0 */
            (void)hipFree(dbuf);
            return 0;
        }
        std::vector<float> img((size_t)W * rows * 4);
        if (hipMemcpy(img.data(), dbuf, img.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
        (void)hipFree(dbuf);
        if (denoise || !feat_out.empty()) { /* whole frames only: the features know no tile */
            if (tiled) {
                std::fprintf(stderr, "rt_render: --denoise / --features-out need the whole frame (no --tile)\n");
                return 1;
            }
            std::vector<float> feat((size_t)W * H * 8), den(img.size());
            rt.renderFeatures(feat.data(), W, H, kernel);
            float fms = 0.0f, dms = 0.0f;
            rt_last_features_ms(rt.handle(), &fms);
            if (denoise) {
                rt.denoise(img.data(), feat.data(), den.data(), W, H, den_params);
                rt_last_denoise_ms(rt.handle(), &dms);
            }
            std::printf("{\"features_ms\": %.4f, \"denoise_ms\": %.4f, \"denoise_passes\": %u}\n", fms, dms,
                        denoise ? den_params.iterations : 0u);
            if (!feat_out.empty()) {
                FILE *f = std::fopen(feat_out.c_str(), "wb");
                if (!f || std::fwrite(feat.data(), 4, feat.size(), f) != feat.size()) return 1;
                std::fclose(f);
            }
            if (denoise && !den_raw.empty()) {
                FILE *f = std::fopen(den_raw.c_str(), "wb");
                if (!f || std::fwrite(den.data(), 4, den.size(), f) != den.size()) return 1;
                std::fclose(f);
            }
            if (denoise && !den_pfm.empty()) {
                FILE *f = std::fopen(den_pfm.c_str(), "wb");
                if (!f) return 1;
                std::fprintf(f, "PF\n%u %u\n-1.0\n", W, H);
                for (int y = (int)H - 1; y >= 0; --y)
                    for (unsigned x = 0; x < W; ++x) std::fwrite(&den[((size_t)y * W + x) * 4], 4, 3, f);
                std::fclose(f);
            }
        }
        if (tonemap) { /* the final shown frame (the filtered one with --denoise) through meter and tone map */
            if (tiled) {
                std::fprintf(stderr, "rt_render: --tonemap needs the whole frame (no --tile)\n");
                return 1;
            }
            std::vector<float> shown = img;
            if (denoise) {
                std::vector<float> feat((size_t)W * H * 8);
                rt.renderFeatures(feat.data(), W, H, kernel);
                rt.denoise(img.data(), feat.data(), shown.data(), W, H, den_params);
            }
            float exposure = 0.0f;
            if (auto_exposure) rt.meterExposure(shown.data(), &exposure, nullptr, W, H, meter_params);
            std::vector<uint32_t> px8((size_t)W * H);
            rt.toneMap(shown.data(), auto_exposure ? &exposure : nullptr, px8.data(), W, H, tone_params);
            std::printf("{\"meter_ms\": %.4f, \"tonemap_ms\": %.4f, \"exposure\": %.9g}\n", auto_exposure ? rt.lastToneMapMs(true) : 0.0f,
                        rt.lastToneMapMs(), auto_exposure ? exposure : tone_params.exposure);
            if (!ppm.empty() && !write_ppm(ppm, px8, W, H)) return 1;
        }
        std::printf("{\"frames\": %u, \"seconds\": %.6f, \"frames_per_sec\": %.4f, \"mrays_per_sec\": %.2f}\n", frames,
                    dt, frames / dt, rays / dt / 1e6);
        if (!raw.empty()) {
            FILE *f = std::fopen(raw.c_str(), "wb");
            if (!f || std::fwrite(img.data(), 4, img.size(), f) != img.size()) return 1;
            std::fclose(f);
        }
        if (!pfm.empty()) { /* PFM: bottom-to-top rows, RGB, little-endian */
            FILE *f = std::fopen(pfm.c_str(), "wb");
            if (!f) return 1;
            std::fprintf(f, "PF\n%u %u\n-1.0\n", W, rows);
            for (int y = (int)rows - 1; y >= 0; --y)
                for (unsigned x = 0; x < W; ++x) std::fwrite(&img[((size_t)y * W + x) * 4], 4, 3, f);
            std::fclose(f);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "rt_render: %s\n", e.what());
        return 1;
    }
    return 0;
}
