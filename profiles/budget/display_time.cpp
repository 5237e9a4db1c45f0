// profiles/budget/display_time.cpp — MEASUREMENT PROGRAM: the host wall time of one
// ProgressiveViewHIP::display() of a resting view (progression rising, nothing converges, no tile stops), in
// one process, four views each on a tracer of its own, one display of each in turn within every round:
//   adaptive   setConverge + setAdaptive alone: the path before there was a budget (its calls are the parent
//              commit's: the accumulation copy, one masked render, the masked moments)
//   rounds_1   setSampleBudget with max_passes 1: one pass, the fold in place of the copy and the moments
//   rounds_2, rounds_4   max_passes 2 and 4 with limits every tile exceeds: every tile traced 2 and 4 times
// Prints one JSON line: per view the median, minimum, maximum and quartiles of --reps displays (ms).
//   hipcc -O2 -std=c++17 -I include -o profiles/budget/display_time profiles/budget/display_time.cpp \
//       -Lpathtracer.cl_amd -lrtmi -Wl,-rpath,'$ORIGIN/../../pathtracer.cl_amd'
//   profiles/budget/display_time [--tris N] [--width W] [--height H] [--reps R] [--warmup K]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ProgressiveViewHIP.hpp"

static rt_sphere sphere(float x, float y, float z)
{
    rt_sphere s;
    std::memset(&s, 0, sizeof(s));
    s.radius = 1.0f;
    s.mat.specExp = s.mat.refExp = 1000000.0f;
    s.mat.ior = 1.0f;
    s.center = {x, y, z};
    return s;
}

int main(int argc, char **argv)
{
    unsigned n_tris = 871414, W = 1920, H = 1080, reps = 20, warmup = 3;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string a = argv[i];
        const unsigned v = (unsigned)std::atoi(argv[i + 1]);
        if (a == "--tris") n_tris = v;
        else if (a == "--width") W = v;
        else if (a == "--height") H = v;
        else if (a == "--reps") reps = v;
        else if (a == "--warmup") warmup = v;
        else return 2;
    }
    try {
        std::vector<float> v(3ull * rt_mesh_vertex_count(n_tris));
        std::vector<int> idx(3ull * n_tris);
        if (rt_make_mesh(n_tris, 0.0f, -2.2f, 0.0f, 2.5f, v.data(), idx.data()) != RT_OK) return 1;
        rt_noise_params never = RayTracerHIP::noiseDefaults();
        never.threshold = 0.0f;
        rt_adaptive_params no_stop = RayTracerHIP::adaptiveDefaults();
        no_stop.min_frames = 1u << 30;
        constexpr int kViews = 4;
        const char *names[kViews] = {"adaptive", "rounds_1", "rounds_2", "rounds_4"};
        const unsigned passes[kViews] = {0, 1, 2, 4};
        std::unique_ptr<RayTracerHIP> rt[kViews];
        std::unique_ptr<ProgressiveViewHIP> view[kViews];
        for (int k = 0; k < kViews; ++k) {
            rt[k].reset(new RayTracerHIP(0));
            rt_sphere s = sphere(-2.0f, -4.0f, -2.0f); /* plymain.cpp's scene in short: a diffuse sphere and the light */
            s.mat.kd = 1.0f;
            s.mat.diffuse = {0.0f, 0.7f, 0.7f};
            rt[k]->addSphere(s);
            s = sphere(0.0f, 4.0f, 2.0f);
            s.radius = 0.5f;
            s.mat.emission_power = 1.0f;
            s.mat.emission = {1.1f, 1.1f, 1.1f};
            rt[k]->addSphere(s);
            rt[k]->setSampleRate(1);
            rt[k]->setMaxPathDepth(6);
            rt[k]->setMesh(v.data(), (unsigned)(v.size() / 3), idx.data(), n_tris);
            view[k].reset(new ProgressiveViewHIP(*rt[k], W, H, RT_KERNEL_TRIS));
            view[k]->setConverge(true, never);
            view[k]->setAdaptive(true, no_stop);
            if (passes[k]) {
                rt_budget_params b = RayTracerHIP::budgetDefaults();
                b.max_passes = passes[k];
                b.limits[0] = 0.0f; /* every tile with any error at all is over every limit */
                b.limits[1] = 1e-30f;
                b.limits[2] = 1e-20f;
                view[k]->setSampleBudget(true, b);
            }
            for (int d = 0; d < 3; ++d) view[k]->display(); /* progression 0, 1, 2: the lists, the schedule, a budget */
        }
        std::vector<double> ms[kViews];
        unsigned rounds_seen[kViews] = {};
        for (unsigned r = 0; r < warmup + reps; ++r)
            for (int k = 0; k < kViews; ++k) {
                const auto t0 = std::chrono::steady_clock::now();
                view[k]->display();
                const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (r >= warmup) ms[k].push_back(dt);
                rounds_seen[k] = view[k]->budgetStats().rounds;
            }
        std::printf("{\"workload\": \"%u triangles, %ux%u, 1 spp a pass, a display of a resting view\", \"reps\": %u", n_tris, W, H, reps);
        for (int m = 0; m < kViews; ++m) {
            std::sort(ms[m].begin(), ms[m].end());
            const size_t n = ms[m].size();
            std::printf(", \"display_%s_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f, \"q1\": %.4f, \"q3\": %.4f, \"rounds\": %u, "
                        "\"tile_passes\": %u}",
                        names[m], (ms[m][(n - 1) / 2] + ms[m][n / 2]) / 2.0, ms[m].front(), ms[m].back(), ms[m][n / 4], ms[m][(3 * n) / 4],
                        rounds_seen[m], view[m]->budgetStats().tile_passes);
        }
        std::printf("}\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "display_time: %s\n", e.what());
        return 1;
    }
    return 0;
}
