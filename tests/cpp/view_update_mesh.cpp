/*
 * view_update_mesh — TEST PROGRAM (tests/test_gpu_refit.py compiles and runs it): the C++ side of
 * the moving mesh, RayTracerHIP::updateMesh / lastMeshUpdate and ProgressiveViewHIP::updateMesh.
 *
 *   view_update_mesh W H n_tris
 *
 * View A shows the mesh for three frames with the temporal and the variance-guided display on,
 * then moves it (updateMesh) and shows two more frames.  View B, on a tracer of its own, shows the
 * same three frames, then gets the moved vertices by a fresh setMesh and forgets its display
 * history the long way (both stages switched off and on again, restart()), takes A's seeds and
 * shows two frames.  After an update nothing of the old geometry may be left in what A displays:
 * its two frames equal B's bit for bit.  (Both views refine the same accumulation buffer: a
 * progressive frame mixes into what the buffer holds, raytracer.cl:234-242, so a view that never
 * showed the old mesh would differ in the mix's rounding.)
 * Exit status 0: equal (and the preconditions hold), 1: not, 3: no GPU or a failed call.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ProgressiveViewHIP.hpp"
#include "RayTracerHIP.hpp"

namespace {

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

/* a diffuse sphere and the mesh scene's light (plymain.cpp:45-111, shortened) */
void add_scene(RayTracerHIP &rt)
{
    rt_sphere s = init_sphere();
    s.center = {-2.0f, -4.0f, -2.0f};
    s.mat.kd = 1.0f;
    s.mat.diffuse = {0.0f, 0.7f, 0.7f};
    rt.addSphere(s);
    s = init_sphere();
    s.center = {0.0f, 4.0f, 2.0f};
    s.radius = 0.5f;
    s.mat.emission_power = 1.0f;
    s.mat.emission = {1.1f, 1.1f, 1.1f};
    rt.addSphere(s);
}

void setup(ProgressiveViewHIP &view)
{
    view.setProgressive(8);
    view.setTemporal(true);
    view.setVarianceGuided(true);
}

bool same(const std::vector<float> &a, const std::vector<float> &b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s W H n_tris\n", argv[0]);
        return 2;
    }
    const unsigned W = (unsigned)std::atoi(argv[1]), H = (unsigned)std::atoi(argv[2]);
    const uint32_t n_tris = (uint32_t)std::atoi(argv[3]);
    try {
        std::vector<float> v0(3ull * rt_mesh_vertex_count(n_tris));
        std::vector<int> idx(3ull * n_tris);
        if (rt_make_mesh(n_tris, 0.0f, -2.2f, 0.0f, 2.5f, v0.data(), idx.data()) != RT_OK) return 3;
        const uint32_t n_verts = (uint32_t)(v0.size() / 3);
        std::vector<float> v1(v0);
        for (uint32_t i = 0; i < n_verts; ++i) { /* a wobble, and a step aside */
            const float *p = &v0[3ull * i];
            v1[3ull * i] = p[0] + 0.15f * std::sin(2.0f * p[1] + 0.3f) + 0.4f;
            v1[3ull * i + 1] = p[1] + 0.15f * std::sin(2.0f * p[2] + 1.1f);
            v1[3ull * i + 2] = p[2] + 0.15f * std::sin(2.0f * p[0] + 2.0f);
        }
        const float target[3] = {0.0f, -4.0f, 0.0f};

        RayTracerHIP a(0);
        add_scene(a);
        a.setSampleRate(1);
        a.setMaxPathDepth(6);
        a.setCameraSpherical(target, 40.0f, 105.0f, 5.0f);
        a.setMesh(v0.data(), n_verts, idx.data(), n_tris);
        ProgressiveViewHIP va(a, W, H, RT_KERNEL_TRIS);
        setup(va);
        for (int i = 0; i < 3; ++i) va.display();
        const std::vector<float> before = va.pixels();
        const bool post = va.updateMesh(v1.data(), n_verts);
        const rt_mesh_update_info up = a.lastMeshUpdate();
        if (up.action != RT_MESH_UPDATE_REFIT || up.reason != RT_REFIT_OK || !(up.area_ratio > 0.0f)) {
            std::fprintf(stderr, "updateMesh: action %u reason %u area_ratio %g\n", up.action, up.reason, up.area_ratio);
            return 1;
        }
        if (post || va.progression() != 0) {
            std::fprintf(stderr, "updateMesh: progression %u, post %d (restart() in mid-accumulation returns false)\n",
                         va.progression(), (int)post);
            return 1;
        }
        uint32_t wp = 0, hp = 0;
        if (rt_seed_layout(a.handle(), &wp, &hp) != RT_OK) return 3;
        std::vector<uint32_t> seeds(2ull * wp * hp);
        if (rt_get_seeds(a.handle(), seeds.data(), seeds.size()) != RT_OK) return 3;
        std::vector<float> fa[2], fb[2];
        for (int i = 0; i < 2; ++i) {
            va.display();
            fa[i] = va.pixels();
        }

        RayTracerHIP b(0);
        add_scene(b);
        b.setSampleRate(1);
        b.setMaxPathDepth(6);
        b.setCameraSpherical(target, 40.0f, 105.0f, 5.0f);
        b.setMesh(v0.data(), n_verts, idx.data(), n_tris);
        ProgressiveViewHIP vb(b, W, H, RT_KERNEL_TRIS);
        setup(vb);
        for (int i = 0; i < 3; ++i) vb.display();
        if (!same(before, vb.pixels())) {
            std::fprintf(stderr, "precondition: the two views differ before the mesh moves\n");
            return 1;
        }
        b.setMesh(v1.data(), n_verts, idx.data(), n_tris);
        vb.setTemporal(false);
        vb.setVarianceGuided(false);
        setup(vb); /* switched on again: features dirty, no history, no moments */
        vb.restart();
        if (rt_set_seeds(b.handle(), seeds.data(), seeds.size()) != RT_OK) return 3;
        for (int i = 0; i < 2; ++i) {
            vb.display();
            fb[i] = vb.pixels();
        }
        /* RayTracerHIP::updateMesh alone, with the vertices the tree already has: a refit, area unchanged */
        b.updateMesh(v1.data(), n_verts);
        if (b.lastMeshUpdate().action != RT_MESH_UPDATE_REFIT || b.lastMeshUpdate().area_ratio != 1.0f) return 1;

        if (same(before, fa[0]) || same(fa[0], fa[1])) {
            std::fprintf(stderr, "precondition: the displayed frames do not differ\n");
            return 1;
        }
        for (int i = 0; i < 2; ++i)
            if (!same(fa[i], fb[i])) {
                size_t n = 0;
                for (size_t k = 0; k < fa[i].size(); ++k) n += std::memcmp(&fa[i][k], &fb[i][k], 4) != 0;
                std::fprintf(stderr, "frame %d after the update differs from the fresh view's in %zu of %zu values\n", i, n,
                             fa[i].size());
                return 1;
            }
        std::printf("ok: refit %.3f ms, area ratio %.6f\n", up.ms, up.area_ratio);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "view_update_mesh: %s\n", e.what());
        return 3;
    }
}
