// profiles/noise/display_time.cpp — MEASUREMENT PROGRAM: the host wall time of one
// ProgressiveViewHIP::display() of a 1-spp frame after a key press, in one process, setConverge off and
// on alternated (a threshold of 0: the view never converges), in two settings:
//   stages   temporal + variance-guided + history trust on: the moments and the variance plane exist
//            anyway, and the step adds the meter and its sixteen-byte readback
//   plain    nothing else on: the step also makes the view keep the accumulation copy, the moments,
//            the features and the variance plane
// Prints one JSON line: per configuration the median, minimum, maximum and quartiles of --reps displays (ms).
//   hipcc -O2 -std=c++17 -I include -o profiles/noise/display_time profiles/noise/display_time.cpp \
//       -Lpathtracer.cl_amd -lrtmi -Wl,-rpath,'$ORIGIN/../../pathtracer.cl_amd'
//   profiles/noise/display_time [--tris N] [--width W] [--height H] [--reps R] [--warmup K]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
        RayTracerHIP rt(0);
        rt_sphere s = sphere(-2.0f, -4.0f, -2.0f); /* plymain.cpp's scene in short: a diffuse sphere and the light */
        s.mat.kd = 1.0f;
        s.mat.diffuse = {0.0f, 0.7f, 0.7f};
        rt.addSphere(s);
        s = sphere(0.0f, 4.0f, 2.0f);
        s.radius = 0.5f;
        s.mat.emission_power = 1.0f;
        s.mat.emission = {1.1f, 1.1f, 1.1f};
        rt.addSphere(s);
        rt.setSampleRate(1);
        rt.setMaxPathDepth(6);
        std::vector<float> v(3ull * rt_mesh_vertex_count(n_tris));
        std::vector<int> idx(3ull * n_tris);
        if (rt_make_mesh(n_tris, 0.0f, -2.2f, 0.0f, 2.5f, v.data(), idx.data()) != RT_OK) return 1;
        rt.setMesh(v.data(), (unsigned)(v.size() / 3), idx.data(), n_tris);
        rt_noise_params never = RayTracerHIP::noiseDefaults();
        never.threshold = 0.0f;
        const char *names[4] = {"stages_off", "stages_on", "plain_off", "plain_on"};
        std::vector<double> ms[4];
        for (int setting = 0; setting < 2; ++setting) {
            ProgressiveViewHIP view(rt, W, H, RT_KERNEL_TRIS);
            if (setting == 0) {
                view.setTemporal(true);
                view.setVarianceGuided(true);
                view.setHistoryTrust(true);
            }
            view.display();
            view.display();
            for (unsigned r = 0; r < warmup + reps; ++r)
                for (int on = 0; on < 2; ++on) {
                    view.setConverge(on != 0, never);
                    view.specialKey(r & 1 ? ProgressiveViewHIP::KEY_LEFT : ProgressiveViewHIP::KEY_RIGHT);
                    const auto t0 = std::chrono::steady_clock::now();
                    view.display();
                    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                    if (r >= warmup) ms[2 * setting + on].push_back(dt);
                }
        }
        std::printf("{\"workload\": \"%u triangles, %ux%u, 1 spp, a display after a key press\", \"reps\": %u", n_tris, W, H, reps);
        for (int m = 0; m < 4; ++m) {
            std::sort(ms[m].begin(), ms[m].end());
            const size_t n = ms[m].size();
            std::printf(", \"display_%s_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f, \"q1\": %.4f, \"q3\": %.4f}", names[m],
                        (ms[m][(n - 1) / 2] + ms[m][n / 2]) / 2.0, ms[m].front(), ms[m].back(), ms[m][n / 4], ms[m][(3 * n) / 4]);
        }
        std::printf("}\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "display_time: %s\n", e.what());
        return 1;
    }
    return 0;
}
