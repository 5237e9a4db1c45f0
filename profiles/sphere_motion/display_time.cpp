// profiles/sphere_motion/display_time.cpp — MEASUREMENT PROGRAM: the host wall time of one
// ProgressiveViewHIP::display() of a 1-spp frame of the main scene after sphere 2 has moved and
// sceneChanged() was called, setTemporal on, in one process, three configurations alternated:
//   drop       nothing else: the history is dropped (what the view did before the carry existed)
//   trust_inf  setHistoryTrust with tolerance +inf: the history is kept where it was and reprojected
//              (the most the view could do before: the reprojection without the warp)
//   carry      setSphereCarry: the warp, then the reprojection
// Prints one JSON line: per configuration the median, minimum and maximum of --reps displays (ms).
//   hipcc -O2 -std=c++17 -I include -o profiles/sphere_motion/display_time profiles/sphere_motion/display_time.cpp \
//       -Lpathtracer.cl_amd -lrtmi -Wl,-rpath,'$ORIGIN/../../pathtracer.cl_amd'
//   profiles/sphere_motion/display_time [--width W] [--height H] [--reps R] [--warmup K]
#include <algorithm>
#include <chrono>
#include <cmath>
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

/* clrt/main.cpp's spheres, sphere 2 moved by (dx, 0, dz) */
static void scene(RayTracerHIP &rt, float dx, float dz)
{
    rt.clearSpheres();
    rt_sphere s = sphere(-2.0f, -4.0f, -2.0f);
    s.mat.kd = 1.0f;
    s.mat.diffuse = {0.0f, 0.7f, 0.7f};
    rt.addSphere(s);
    s = sphere(2.0f, -3.0f, 2.0f);
    s.mat.ks = 0.2f;
    s.mat.kt = 0.8f;
    s.mat.extinction = {0.99f, 0.95f, 0.95f};
    s.mat.ior = 1.1f;
    rt.addSphere(s);
    s = sphere(0.0f + dx, -4.0f, 0.0f + dz);
    s.mat.ks = 1.0f;
    rt.addSphere(s);
    s = sphere(2.0f, -4.0f, -2.0f);
    s.mat.kd = 0.2f;
    s.mat.ks = 0.8f;
    s.mat.diffuse = {0.7f, 0.7f, 0.0f};
    s.mat.specExp = 100.0f;
    rt.addSphere(s);
    s = sphere(-2.0f, -4.0f, 2.0f);
    s.mat.kd = 0.6f;
    s.mat.ks = 0.4f;
    s.mat.diffuse = {0.7f, 0.0f, 0.8f};
    s.mat.specExp = 1000.0f;
    rt.addSphere(s);
    s = sphere(2.2f, 1.0f, 2.0f);
    s.radius = 0.5f;
    s.mat.emission_power = 1.0f;
    s.mat.emission = {1.8f, 1.8f, 1.8f};
    rt.addSphere(s);
}

int main(int argc, char **argv)
{
    unsigned W = 1920, H = 1080, reps = 20, warmup = 3;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string a = argv[i];
        const unsigned v = (unsigned)std::atoi(argv[i + 1]);
        if (a == "--width") W = v;
        else if (a == "--height") H = v;
        else if (a == "--reps") reps = v;
        else if (a == "--warmup") warmup = v;
        else return 2;
    }
    try {
        RayTracerHIP rt(0);
        scene(rt, 0.0f, 0.0f);
        rt.setSampleRate(1);
        rt.setMaxPathDepth(6);
        const float target[3] = {0.0f, -4.0f, 0.0f};
        rt.setCameraSpherical(target, 14.0f, 118.0f, 5.0f);
        ProgressiveViewHIP view(rt, W, H, RT_KERNEL_SPHERES);
        view.setTemporal(true);
        rt_trust_params all = RayTracerHIP::trustDefaults();
        all.tolerance = INFINITY;
        const char *names[3] = {"drop", "trust_inf", "carry"};
        std::vector<double> ms[3];
        view.display();
        view.display();
        for (unsigned r = 0; r < warmup + reps; ++r)
            for (int m = 0; m < 3; ++m) {
                view.setHistoryTrust(m == 1, all);
                view.setSphereCarry(m == 2);
                view.display(); /* a frame to carry (and, with the carry on, its sphere list) */
                scene(rt, (r + m) & 1 ? 0.25f : 0.0f, (r + m) & 1 ? 0.1f : 0.0f);
                view.sceneChanged();
                const auto t0 = std::chrono::steady_clock::now();
                view.display();
                const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (r >= warmup) ms[m].push_back(dt);
            }
        std::printf("{\"workload\": \"main scene, %ux%u, 1 spp, temporal, display() after a move of sphere 2\", \"reps\": %u", W, H, reps);
        for (int m = 0; m < 3; ++m) {
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
