/*
 * RayTracerHIP.hpp — header-only C++ host class over the C-ABI (librtmi.so).
 *
 * The drop-in for the reference's C++ host API: the public surface of
 * RayTracer (clrt/RayTracer.h:51-70) and RayTracerCL::rayTrace
 * (clrt/RayTracerCL.h:111-112) with the same method names, argument meaning,
 * defaults (fov 53, sampleRate 8, maxPathDepth 4: RayTracer.cpp:16-22) and
 * RGBA32F framebuffer layout.  Like the reference (which throws cl::Error),
 * failures throw — here std::runtime_error carrying the C-ABI status text.
 *
 * The scene is re-uploaded only when it changed, as RayTracerCL does when the
 * sphere count changes (RayTracerCL.cpp:251-264).
 *
 * Source compatibility with the reference's callers (clrt/main.cpp, plymain.cpp,
 * GlutCLWindow.cpp): when the reference's own headers are on the include path
 * (-I<reference>/clrt/ocl for geometry.h, -I<reference>/include for gmtl), the
 * overloads taking its types are compiled in:
 *   addSphere / removeSphere (Sphere const &)              RayTracer.h:68-69
 *   setCameraMatrix(gmtl::Matrix44f const &)               RayTracer.h:56
 *   setCameraSpherical(gmtl::Point3f const &, el, az, d)   RayTracer.h:57
 * so `window.rayTracer.addSphere(sphere)` and
 * `setCameraSpherical(gmtl::Point3f(0, -4, -0), 14.0f, 118.0f, 5)` compile unchanged
 * (tests/cpp/ref_main_replay.cpp replays main.cpp / plymain.cpp through this class).
 * Define RT_HIP_NO_REFERENCE_TYPES to leave them out.
 */
#ifndef RAYTRACER_HIP_HPP
#define RAYTRACER_HIP_HPP

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "pathtracer_rt.h"

#if !defined(RT_HIP_NO_REFERENCE_TYPES) && defined(__has_include)
#if __has_include("geometry.h") && __has_include(<CL/cl.h>)
#include "geometry.h" /* clrt/ocl/geometry.h: Sphere, material_t, vec3 */
#define RT_HIP_HAVE_REF_GEOMETRY 1
#endif
#if __has_include(<gmtl/Matrix.h>) && __has_include(<gmtl/Point.h>)
#include <gmtl/Matrix.h>
#include <gmtl/Point.h>
#define RT_HIP_HAVE_GMTL 1
#endif
#endif

class RayTracerHIP {
public:
    explicit RayTracerHIP(int device = 0)
    {
        check(rt_create(device, &ctx_), "rt_create");
        check(rt_set_params(ctx_, sampleRate_, maxPathDepth_), "rt_set_params");
    }
    ~RayTracerHIP()
    {
        if (ctx_) rt_destroy(ctx_);
    }
    RayTracerHIP(const RayTracerHIP &) = delete;
    RayTracerHIP &operator=(const RayTracerHIP &) = delete;

    /* ---- camera: RayTracer.h:56-60 ---- */
    /* 4x4 matrix, column-major (gmtl's storage order). */
    void setCameraMatrix(const float m_colmajor[16]) { check(rt_set_view_matrix(ctx_, m_colmajor), "setCameraMatrix"); }
    void setCameraSpherical(const float target[3], float elevationDeg, float azimuthDeg, float distance)
    {
        check(rt_set_camera_spherical(ctx_, target[0], target[1], target[2], elevationDeg, azimuthDeg, distance),
              "setCameraSpherical");
    }
    void setFoVAngle(float fovDeg)
    {
        fov_ = fovDeg;
        check(rt_set_fov(ctx_, fovDeg), "setFoVAngle");
    }
    float getFoVAngle() const { return fov_; }
#ifdef RT_HIP_HAVE_GMTL
    /* gmtl stores matrices column-major (gmtl/Matrix.h: getData()), the order
       rt_set_view_matrix takes. */
    void setCameraMatrix(gmtl::Matrix44f const &mat) { setCameraMatrix(mat.getData()); }
    void setCameraSpherical(gmtl::Point3f const &target, float elevationDeg, float azimuthDeg, float distance)
    {
        const float t[3] = {target[0], target[1], target[2]};
        setCameraSpherical(t, elevationDeg, azimuthDeg, distance);
    }
#endif

    /* ---- settings: RayTracer.h:62-66 ---- */
    void setSampleRate(unsigned s)
    {
        sampleRate_ = s;
        check(rt_set_params(ctx_, sampleRate_, maxPathDepth_), "setSampleRate");
    }
    unsigned getSampleRate() const { return sampleRate_; }
    void setMaxPathDepth(unsigned d)
    {
        maxPathDepth_ = d;
        check(rt_set_params(ctx_, sampleRate_, maxPathDepth_), "setMaxPathDepth");
    }
    unsigned getMaxPathDepth() const { return maxPathDepth_; }

    /* ---- scene: RayTracer.h:68-70 ---- */
    void addSphere(const rt_sphere &s)
    {
        spheres_.push_back(s);
        dirty_ = true;
    }
    /* The reference leaves removeSphere a stub (RayTracer.cpp:55-58); this removes
       the first byte-identical sphere. */
    void removeSphere(const rt_sphere &s)
    {
        for (size_t i = 0; i < spheres_.size(); ++i)
            if (std::memcmp(&spheres_[i], &s, sizeof(rt_sphere)) == 0) {
                spheres_.erase(spheres_.begin() + (long)i);
                dirty_ = true;
                return;
            }
    }
#ifdef RT_HIP_HAVE_REF_GEOMETRY
    /* The reference's Sphere (geometry.h:156-163), copied field by field into the
       80-byte rt_sphere record the kernels read (same members, same order). */
    static rt_sphere to_rt(Sphere const &r)
    {
        rt_sphere s;
        s.mat.diffuse = {r.mat.diffuse.x, r.mat.diffuse.y, r.mat.diffuse.z};
        s.mat.kd = r.mat.kd;
        s.mat.extinction = {r.mat.extinction.x, r.mat.extinction.y, r.mat.extinction.z};
        s.mat.kt = r.mat.kt;
        s.mat.emission = {r.mat.emission.x, r.mat.emission.y, r.mat.emission.z};
        s.mat.emission_power = r.mat.emission_power;
        s.mat.ks = r.mat.ks;
        s.mat.specExp = r.mat.specExp;
        s.mat.ior = r.mat.ior;
        s.mat.refExp = r.mat.refExp;
        s.center = {r.center.x, r.center.y, r.center.z};
        s.radius = r.radius;
        return s;
    }
    void addSphere(Sphere const &sphere) { addSphere(to_rt(sphere)); }
    void removeSphere(Sphere const &sphere) { removeSphere(to_rt(sphere)); }
#endif
    void clearSpheres()
    {
        spheres_.clear();
        dirty_ = true;
    }

    /* ---- mesh for raytrace_tris (raytracer.cl:184-188); builds the BVH, its cost area leaning
       toward the lights of the spheres added so far (uploaded first; culling only) ---- */
    void setMesh(const float *verts_xyz, unsigned n_verts, const int *idx, unsigned n_tris)
    {
        flushScene();
        check(rt_set_mesh(ctx_, verts_xyz, n_verts, idx, n_tris), "setMesh");
    }
    /* New positions for the vertices of the last setMesh (rt_update_mesh: a refit of both trees on
       the device, or a rebuild where a refit cannot stand for a build; lastMeshUpdate() says which).
       flags: RT_MESH_VERTS_DEVICE when verts_xyz is device memory. */
    void updateMesh(const float *verts_xyz, uint32_t n_verts, int flags = 0)
    {
        check(rt_update_mesh(ctx_, verts_xyz, n_verts, flags), "updateMesh");
    }
    /* The next host-built setMesh keeps every triangle, so that every later updateMesh refits. */
    void setMeshDynamic(bool on) { check(rt_set_mesh_dynamic(ctx_, on ? 1 : 0), "setMeshDynamic"); }
    rt_mesh_update_info lastMeshUpdate() const
    {
        rt_mesh_update_info i;
        check(rt_last_mesh_update(ctx_, &i), "lastMeshUpdate");
        return i;
    }
    void setTraversal(int traversal) { check(rt_set_traversal(ctx_, traversal), "setTraversal"); }
    /* BVH builder for the next setMesh: RT_BUILD_HOST (binned SAH), RT_BUILD_GPU (LBVH) or
       RT_BUILD_GPU_PLOC (PLOC: device-built, merged by surface area). */
    void setBuilder(int builder) { check(rt_set_builder(ctx_, builder), "setBuilder"); }
    /* Options of the device builders for the next setMesh (RT_BUILD_OPT_LIGHTS: never-hit
       triangles left out, and a shadow tree split by what can occlude the lights). */
    void setBuildOptions(uint32_t opts) { check(rt_set_build_options(ctx_, opts), "setBuildOptions"); }
    uint32_t buildOptions() const
    {
        uint32_t o = 0;
        check(rt_get_build_options(ctx_, &o), "buildOptions");
        return o;
    }
    /* How the device builders collapse their binary tree for the next setMesh: RT_COLLAPSE_GREEDY
       (default) or RT_COLLAPSE_SAH (the host build's rule). */
    void setCollapse(int mode) { check(rt_set_collapse(ctx_, mode), "setCollapse"); }
    int collapse() const
    {
        int m = RT_COLLAPSE_GREEDY;
        check(rt_get_collapse(ctx_, &m), "collapse");
        return m;
    }

    /* plymain.cpp's PLYLoader (PLYLoader.cpp:4-90) with the mesh actually handed over:
       read a PLY file, optionally normalise it (extent 3, resting on y = -5, centred on
       x = z = 0) and set it as the mesh. */
    void setMeshFromPly(const char *path, bool normalize = true)
    {
        rt_ply *ply = nullptr;
        uint32_t nv = 0, nt = 0;
        if (rt_ply_open(path, &ply, &nv, &nt) != RT_OK)
            throw std::runtime_error(std::string("setMeshFromPly: ") + rt_ply_last_error());
        std::vector<float> v(3ull * nv);
        std::vector<int32_t> idx(3ull * nt);
        const int r = rt_ply_read(ply, v.data(), idx.data());
        rt_ply_close(ply);
        check(r, "setMeshFromPly: read");
        if (normalize) check(rt_normalize_mesh(v.data(), nv, 3.0f, -5.0f), "setMeshFromPly: normalise");
        setMesh(v.data(), nv, idx.data(), nt);
    }

    /* ---- RayTracerCL::rayTrace(cl_mem*, W, H, progression) ----
       `buff` is W*H*4 floats; a device pointer when on_device, else host memory. */
    void rayTrace(float *buff, unsigned width, unsigned height, unsigned progression,
                  int kernel = RT_KERNEL_SPHERES, bool on_device = false, const rt_tile *tile = nullptr)
    {
        if (dirty_) {
            check(rt_set_spheres(ctx_, spheres_.empty() ? nullptr : spheres_.data(), (uint32_t)spheres_.size()),
                  "scene upload");
            dirty_ = false;
        }
        check(rt_render(ctx_, buff, width, height, progression, kernel, tile, on_device ? RT_OUT_DEVICE : 0),
              "rayTrace");
    }

    /* Upload a changed sphere list now (rayTrace does it itself; callers that drive the
       C-ABI directly with handle(), e.g. rt_comm_render, call this first). */
    void flushScene()
    {
        if (dirty_) {
            check(rt_set_spheres(ctx_, spheres_.empty() ? nullptr : spheres_.data(), (uint32_t)spheres_.size()),
                  "scene upload");
            dirty_ = false;
        }
    }

    /* Blocking readback of the last frame into host memory (the non-sharing display
       path, GlutCLWindow.cpp:214-225); n_floats = capacity of `host`. */
    void read(float *host, size_t n_floats) { check(rt_read(ctx_, host, n_floats), "read"); }

    /* ---- first-hit features and the display denoiser (pathtracer_rt.h; nothing in the
       reference corresponds to them).  None of them changes a render's state. ---- */
    /* The pixel-centre camera rays of a W x H frame under the current camera, row-major. */
    std::vector<rt_ray> primaryRays(unsigned width, unsigned height) const
    {
        rt_camera cam;
        check(rt_get_camera(ctx_, width, &cam), "primaryRays: camera");
        std::vector<rt_ray> rays((size_t)width * height);
        check(rt_primary_rays(&cam, width, height, rays.data()), "primaryRays");
        return rays;
    }
    /* feat: 2 planes of W*H float4, (P, t) then (N, surface id bits); device or host memory. */
    void renderFeatures(float *feat, unsigned width, unsigned height, int kernel = RT_KERNEL_SPHERES,
                        bool on_device = false)
    {
        flushScene();
        check(rt_render_features(ctx_, feat, width, height, kernel, on_device ? RT_OUT_DEVICE : 0), "renderFeatures");
    }
    static rt_denoise_params denoiseDefaults()
    {
        rt_denoise_params p;
        rt_denoise_defaults(&p);
        return p;
    }
    /* Edge-avoiding a-trous filter of `in` guided by `feat` into `out` (may be `in`); all three
       device pointers when on_device, else host memory. */
    void denoise(const float *in, const float *feat, float *out, unsigned width, unsigned height,
                 const rt_denoise_params &params = denoiseDefaults(), bool on_device = false)
    {
        check(rt_denoise(ctx_, in, feat, out, width, height, &params, on_device ? RT_OUT_DEVICE : 0), "denoise");
    }

    /* ---- temporal reprojection of the displayed frame (pathtracer_rt.h) ---- */
    rt_camera getCamera(unsigned width) const
    {
        rt_camera cam;
        check(rt_get_camera(ctx_, width, &cam), "getCamera");
        return cam;
    }
    static rt_reproject_params reprojectDefaults()
    {
        rt_reproject_params p;
        rt_reproject_defaults(&p);
        return p;
    }
    /* Carry the previous view's displayed frame (prev_rgba, its history lengths prev_len, its
       features and camera) over to the view of cur_feat: out_rgba / out_len, apart from prev_*. */
    void reproject(const float *prev_rgba, const float *prev_len, const float *prev_feat, const rt_camera &prev_cam,
                   const float *cur_feat, float *out_rgba, float *out_len, unsigned width, unsigned height,
                   const rt_reproject_params &params = reprojectDefaults(), bool on_device = false)
    {
        check(rt_reproject(ctx_, prev_rgba, prev_len, prev_feat, &prev_cam, cur_feat, out_rgba, out_len, width, height,
                           &params, on_device ? RT_OUT_DEVICE : 0),
              "reproject");
    }
    /* Blend the carried history with the accumulation buffer `cur` of n_cur frames; out_* may be hist_*. */
    void temporalMerge(const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur,
                       float max_history, float *out_rgba, float *out_len, unsigned width, unsigned height,
                       bool on_device = false)
    {
        check(rt_temporal_merge(ctx_, hist_rgba, hist_len, cur_rgba, n_cur, max_history, out_rgba, out_len, width, height,
                                on_device ? RT_OUT_DEVICE : 0),
              "temporalMerge");
    }
    /* Device time of the last reprojection kernel, or (merge) of the last merge kernel, ms. */
    float lastReprojectMs(bool merge = false) const
    {
        float ms = 0.0f;
        check(rt_last_reproject_ms(ctx_, merge ? nullptr : &ms, merge ? &ms : nullptr), "lastReprojectMs");
        return ms;
    }

    /* ---- lag-adaptive trust of the carried history (pathtracer_rt.h) ---- */
    static rt_trust_params trustDefaults()
    {
        rt_trust_params p;
        rt_trust_defaults(&p);
        return p;
    }
    /* The history length each pixel of the carried history (hist_rgba, hist_len) still deserves against
       the accumulation buffer cur_rgba of n_cur frames: out_len (may be hist_len), temporalMerge's hist_len. */
    void historyTrust(const float *hist_rgba, const float *hist_len, const float *cur_rgba, float n_cur, const float *feat,
                      float *out_len, unsigned width, unsigned height, const rt_trust_params &params = trustDefaults(),
                      bool on_device = false)
    {
        check(rt_history_trust(ctx_, hist_rgba, hist_len, cur_rgba, n_cur, feat, out_len, width, height, &params,
                               on_device ? RT_OUT_DEVICE : 0),
              "historyTrust");
    }
    float lastTrustMs() const
    {
        float ms = 0.0f;
        check(rt_last_trust_ms(ctx_, &ms), "lastTrustMs");
        return ms;
    }

    /* ---- carrying the displayed frame across updateMesh (pathtracer_rt.h) ---- */
    /* The vertices of the current mesh as the trees hold them (the last successful setMesh / updateMesh). */
    void meshPose(float *out_verts_xyz, uint32_t n_verts, bool on_device = false) const
    {
        check(rt_mesh_pose(ctx_, out_verts_xyz, n_verts, on_device ? RT_OUT_DEVICE : 0), "meshPose");
    }
    /* cur_feat rewritten into the earlier pose prev_verts_xyz of the same mesh: out_feat (may be cur_feat),
       reproject's cur_feat across an updateMesh. */
    void warpFeatures(const float *cur_feat, const float *prev_verts_xyz, uint32_t n_verts, float *out_feat, unsigned width,
                      unsigned height, bool on_device = false)
    {
        check(rt_warp_features(ctx_, cur_feat, prev_verts_xyz, n_verts, out_feat, width, height, on_device ? RT_OUT_DEVICE : 0),
              "warpFeatures");
    }
    float lastWarpMs() const
    {
        float ms = 0.0f;
        check(rt_last_warp_ms(ctx_, &ms), "lastWarpMs");
        return ms;
    }

    /* ---- carrying the displayed frame across sphere moves (pathtracer_rt.h) ---- */
    /* The sphere list as added (uploaded at the next render or display call, if it changed). */
    const std::vector<rt_sphere> &spheres() const { return spheres_; }
    /* cur_feat with every sphere pixel's hit point put back on sphere i of prev_spheres: out_feat (may be
       cur_feat), reproject's cur_feat across a change of the sphere list that keeps its order. */
    void warpFeaturesSpheres(const float *cur_feat, const rt_sphere *prev_spheres, uint32_t n_prev, float *out_feat,
                             unsigned width, unsigned height, bool on_device = false)
    {
        flushScene();
        check(rt_warp_features_spheres(ctx_, cur_feat, prev_spheres, n_prev, out_feat, width, height,
                                       on_device ? RT_OUT_DEVICE : 0),
              "warpFeaturesSpheres");
    }
    float lastSphereWarpMs() const
    {
        float ms = 0.0f;
        check(rt_last_sphere_warp_ms(ctx_, &ms), "lastSphereWarpMs");
        return ms;
    }

    /* ---- variance-guided display filter (pathtracer_rt.h) ---- */
    static rt_denoise_var_params denoiseVarDefaults()
    {
        rt_denoise_var_params p;
        rt_denoise_var_defaults(&p);
        return p;
    }
    /* Fold the frame between the accumulation buffers prev_rgba (a copy taken before it) and cur_rgba
       (after it, n_cur = max(progression, 1) frames) into the view's luminance moments; mom_out may
       be mom_in; n_cur == 1 reads neither prev_rgba nor mom_in. */
    void momentsAccumulate(const float *prev_rgba, const float *cur_rgba, float n_cur, const float *mom_in,
                           float *mom_out, unsigned width, unsigned height, bool on_device = false)
    {
        check(rt_moments_accumulate(ctx_, prev_rgba, cur_rgba, n_cur, mom_in, mom_out, width, height,
                                    on_device ? RT_OUT_DEVICE : 0),
              "momentsAccumulate");
    }
    /* The variance of the displayed luminance (one plane of W*H floats) from the moments frame, the
       history lengths and, where those are short, the frame about to be displayed. */
    void variance(const float *disp_rgba, const float *mom_rgba, const float *len, const float *feat, float *out_var,
                  unsigned width, unsigned height, const rt_denoise_var_params &params = denoiseVarDefaults(),
                  bool on_device = false)
    {
        check(rt_variance(ctx_, disp_rgba, mom_rgba, len, feat, out_var, width, height, &params,
                          on_device ? RT_OUT_DEVICE : 0),
              "variance");
    }
    /* Variance-guided a-trous filter of `in` with its variance plane into `out` (may be `in`) and
       out_var (may be in_var, or NULL). */
    void denoiseVar(const float *in, const float *in_var, const float *feat, float *out, float *out_var, unsigned width,
                    unsigned height, const rt_denoise_var_params &params = denoiseVarDefaults(), bool on_device = false)
    {
        check(rt_denoise_var(ctx_, in, in_var, feat, out, out_var, width, height, &params, on_device ? RT_OUT_DEVICE : 0),
              "denoiseVar");
    }
    /* Device time of the last moments kernel (0), variance kernel (1) or rt_denoise_var (2), ms. */
    float lastVarianceMs(int which = 2) const
    {
        float ms = 0.0f;
        check(rt_last_variance_ms(ctx_, which == 0 ? &ms : nullptr, which == 1 ? &ms : nullptr,
                                  which == 2 ? &ms : nullptr),
              "lastVarianceMs");
        return ms;
    }

    /* ---- tone-mapped 8-bit display output with auto-exposure (pathtracer_rt.h) ---- */
    static rt_tonemap_params toneMapDefaults()
    {
        rt_tonemap_params p;
        rt_tonemap_defaults(&p);
        return p;
    }
    static rt_meter_params meterDefaults()
    {
        rt_meter_params p;
        rt_meter_defaults(&p);
        return p;
    }
    /* Meter the RGBA32F frame: *exposure_io is read as the previous exposure (not positive: none) and
       written as the new one; hist_out: NULL, or RT_METER_BINS counts.  sync = false (device buffers): enqueued
       on the tracer's stream without a wait — a toneMap that follows is ordered after it. */
    void meterExposure(const float *rgba, float *exposure_io, uint32_t *hist_out, unsigned width, unsigned height,
                       const rt_meter_params &params = meterDefaults(), bool on_device = false, bool sync = true)
    {
        const int flags = on_device ? RT_OUT_DEVICE : 0;
        check(sync ? rt_meter_exposure(ctx_, rgba, exposure_io, hist_out, width, height, &params, flags)
                   : rt_meter_exposure_async(ctx_, rgba, exposure_io, hist_out, width, height, &params, flags, nullptr),
              "meterExposure");
    }
    /* Tone-map the RGBA32F frame into out_rgba8 (W*H words, GL_RGBA / GL_UNSIGNED_BYTE in memory) under
       *exposure (as meterExposure wrote it), or with NULL under params.exposure. */
    void toneMap(const float *rgba, const float *exposure, uint32_t *out_rgba8, unsigned width, unsigned height,
                 const rt_tonemap_params &params = toneMapDefaults(), bool on_device = false)
    {
        check(rt_tonemap(ctx_, rgba, exposure, out_rgba8, width, height, &params, on_device ? RT_OUT_DEVICE : 0), "toneMap");
    }
    /* Device time of the last tone-map kernel, or (meter) of the last meter, ms. */
    float lastToneMapMs(bool meter = false) const
    {
        float ms = 0.0f;
        check(rt_last_tonemap_ms(ctx_, meter ? &ms : nullptr, meter ? nullptr : &ms), "lastToneMapMs");
        return ms;
    }
    /* (no counterpart in the reference) the noise meter */
    static rt_noise_params noiseDefaults()
    {
        rt_noise_params p;
        rt_noise_defaults(&p);
        return p;
    }
    /* Meter the RGBA32F frame with the variance plane of its luminance (variance's output): *stats_out
       the level and the counts; tiles_out: NULL, or ceil(W/8) ceil(H/8) pairs (mean, max); hist_out: NULL,
       or RT_METER_BINS counts.  sync = false (device buffers): enqueued on the tracer's stream without a wait. */
    void noiseMeter(const float *rgba, const float *var, rt_noise_stats *stats_out, float *tiles_out, uint32_t *hist_out,
                    unsigned width, unsigned height, const rt_noise_params &params = noiseDefaults(), bool on_device = false,
                    bool sync = true)
    {
        const int flags = on_device ? RT_OUT_DEVICE : 0;
        check(sync ? rt_noise_meter(ctx_, rgba, var, stats_out, tiles_out, hist_out, width, height, &params, flags)
                   : rt_noise_meter_async(ctx_, rgba, var, stats_out, tiles_out, hist_out, width, height, &params, flags, nullptr),
              "noiseMeter");
    }
    /* Device time of the last noise meter, ms. */
    float lastNoiseMs() const
    {
        float ms = 0.0f;
        check(rt_last_noise_ms(ctx_, &ms), "lastNoiseMs");
        return ms;
    }
    /* (no counterpart in the reference) adaptive sampling on the tile map */
    static rt_adaptive_params adaptiveDefaults()
    {
        rt_adaptive_params p;
        rt_adaptive_defaults(&p);
        return p;
    }
    /* The stop plane (a word per 8x8 tile, 0 = rendered) that masks the raytrace_tris renders of width x
       height from now on; NULL clears it.  A host plane is copied; a device plane is borrowed and read at
       every render. */
    void setTileStop(const uint32_t *stop, unsigned width = 0, unsigned height = 0, bool on_device = false)
    {
        check(rt_set_tile_stop(ctx_, stop, width, height, on_device ? RT_OUT_DEVICE : 0), "setTileStop");
    }
    /* The stop rule on noiseMeter's tile map: stop_io updated in place, *stats_out the counts.  sync = false
       (device buffers): enqueued on the tracer's stream without a wait. */
    void tileStopSelect(const float *tiles_mean_max, uint32_t *stop_io, uint32_t n_frames, rt_adaptive_stats *stats_out,
                        unsigned width, unsigned height, const rt_adaptive_params &params = adaptiveDefaults(),
                        bool on_device = false, bool sync = true)
    {
        const int flags = on_device ? RT_OUT_DEVICE : 0;
        check(sync ? rt_tile_stop_select(ctx_, tiles_mean_max, stop_io, n_frames, stats_out, width, height, &params, flags)
                   : rt_tile_stop_select_async(ctx_, tiles_mean_max, stop_io, n_frames, stats_out, width, height, &params,
                                               flags, nullptr),
              "tileStopSelect");
    }
    /* momentsAccumulate under a stop plane, with the per-pixel history lengths `variance` takes. */
    void momentsAccumulateTiles(const float *prev_rgba, const float *cur_rgba, float n_cur, const float *mom_in,
                                float *mom_out, const uint32_t *stop, float *len_out, unsigned width, unsigned height,
                                bool on_device = false)
    {
        check(rt_moments_accumulate_tiles(ctx_, prev_rgba, cur_rgba, n_cur, mom_in, mom_out, stop, len_out, width, height,
                                          on_device ? RT_OUT_DEVICE : 0),
              "momentsAccumulateTiles");
    }
    /* Device time of the last stop rule, or (order) of the last masked order kernel, ms. */
    float lastAdaptiveMs(bool order = false) const
    {
        float ms = 0.0f;
        check(rt_last_adaptive_ms(ctx_, order ? nullptr : &ms, order ? &ms : nullptr), "lastAdaptiveMs");
        return ms;
    }
    /* (no counterpart in the reference) per-tile sample counts */
    static rt_budget_params budgetDefaults()
    {
        rt_budget_params p;
        rt_budget_defaults(&p);
        return p;
    }
    /* The fold of a frame's own sample into acc_rgba, a weight per 8x8 tile from count_io (updated in place): the
       tiles whose word of `passes` exceeds `pass` (passes NULL: all).  The one display-side call that writes an
       accumulation buffer.  sync = false (device buffers): enqueued on the tracer's stream without a wait. */
    void foldTiles(const float *sample_rgba, float *acc_rgba, uint32_t *count_io, const uint32_t *passes, uint32_t pass,
                   const float *mom_in, float *mom_out, float *len_out, unsigned width, unsigned height, bool on_device = false,
                   bool sync = true)
    {
        const int flags = on_device ? RT_OUT_DEVICE : 0;
        check(sync ? rt_fold_tiles(ctx_, sample_rgba, acc_rgba, count_io, passes, pass, mom_in, mom_out, len_out, width, height, flags)
                   : rt_fold_tiles_async(ctx_, sample_rgba, acc_rgba, count_io, passes, pass, mom_in, mom_out, len_out, width,
                                         height, flags, nullptr),
              "foldTiles");
    }
    /* The budget rule on noiseMeter's tile map: passes_out[t] = 0 for a stopped tile, else 1 + the limits its mean
       lies above; *stats_out the counts. */
    void tileBudget(const float *tiles_mean_max, const uint32_t *stop, uint32_t *passes_out, rt_budget_stats *stats_out,
                    unsigned width, unsigned height, const rt_budget_params &params = budgetDefaults(), bool on_device = false,
                    bool sync = true)
    {
        const int flags = on_device ? RT_OUT_DEVICE : 0;
        check(sync ? rt_tile_budget(ctx_, tiles_mean_max, stop, passes_out, stats_out, width, height, &params, flags)
                   : rt_tile_budget_async(ctx_, tiles_mean_max, stop, passes_out, stats_out, width, height, &params, flags, nullptr),
              "tileBudget");
    }
    /* The stop plane of pass `pass`: 0 (rendered) for a live tile whose passes exceed it, else 1. */
    void tilePassMask(const uint32_t *stop, const uint32_t *passes, uint32_t pass, uint32_t *mask_out, unsigned width,
                      unsigned height, bool on_device = false, bool sync = true)
    {
        const int flags = on_device ? RT_OUT_DEVICE : 0;
        check(sync ? rt_tile_pass_mask(ctx_, stop, passes, pass, mask_out, width, height, flags)
                   : rt_tile_pass_mask_async(ctx_, stop, passes, pass, mask_out, width, height, flags, nullptr),
              "tilePassMask");
    }
    /* Device time of the last fold (0), budget rule (1) or pass mask (2), ms. */
    float lastBudgetMs(int which = 0) const
    {
        float ms = 0.0f;
        check(rt_last_budget_ms(ctx_, which == 0 ? &ms : nullptr, which == 1 ? &ms : nullptr, which == 2 ? &ms : nullptr),
              "lastBudgetMs");
        return ms;
    }
    /* (no counterpart in the reference) adaptive sampling under the temporal stage */
    /* temporalMerge with the accumulation buffer's frame count per pixel (cur_len: under 1 reads as 1). */
    void temporalMergeLen(const float *hist_rgba, const float *hist_len, const float *cur_rgba, const float *cur_len,
                          float max_history, float *out_rgba, float *out_len, unsigned width, unsigned height,
                          bool on_device = false, bool sync = true)
    {
        const int flags = on_device ? RT_OUT_DEVICE : 0;
        check(sync ? rt_temporal_merge_len(ctx_, hist_rgba, hist_len, cur_rgba, cur_len, max_history, out_rgba, out_len, width,
                                           height, flags)
                   : rt_temporal_merge_len_async(ctx_, hist_rgba, hist_len, cur_rgba, cur_len, max_history, out_rgba, out_len,
                                                 width, height, flags, nullptr),
              "temporalMergeLen");
    }
    /* historyTrust with the frame count of each pixel's own test taken from cur_len. */
    void historyTrustLen(const float *hist_rgba, const float *hist_len, const float *cur_rgba, const float *cur_len,
                         const float *feat, float *out_len, unsigned width, unsigned height,
                         const rt_trust_params &params = trustDefaults(), bool on_device = false, bool sync = true)
    {
        const int flags = on_device ? RT_OUT_DEVICE : 0;
        check(sync ? rt_history_trust_len(ctx_, hist_rgba, hist_len, cur_rgba, cur_len, feat, out_len, width, height, &params,
                                          flags)
                   : rt_history_trust_len_async(ctx_, hist_rgba, hist_len, cur_rgba, cur_len, feat, out_len, width, height,
                                                &params, flags, nullptr),
              "historyTrustLen");
    }
    /* Per 8x8 tile the shortest of the lengths `len` among its pixels that met a surface (feat NULL: among all). */
    void tileLenMin(const float *len, const float *feat, float *tiles_out, unsigned width, unsigned height, bool on_device = false,
                    bool sync = true)
    {
        const int flags = on_device ? RT_OUT_DEVICE : 0;
        check(sync ? rt_tile_len_min(ctx_, len, feat, tiles_out, width, height, flags)
                   : rt_tile_len_min_async(ctx_, len, feat, tiles_out, width, height, flags, nullptr),
              "tileLenMin");
    }
    float lastTileLenMs() const
    {
        float ms = 0.0f;
        check(rt_last_tile_len_ms(ctx_, &ms), "lastTileLenMs");
        return ms;
    }
    /* tileStopSelect with the frame gate per tile: tile_frames (tileLenMin's tiles_out) against params.min_frames. */
    void tileStopSelectFrames(const float *tiles_mean_max, const float *tile_frames, uint32_t *stop_io, uint32_t n_frames,
                              rt_adaptive_stats *stats_out, unsigned width, unsigned height,
                              const rt_adaptive_params &params = adaptiveDefaults(), bool on_device = false, bool sync = true)
    {
        const int flags = on_device ? RT_OUT_DEVICE : 0;
        check(sync ? rt_tile_stop_select_frames(ctx_, tiles_mean_max, tile_frames, stop_io, n_frames, stats_out, width, height,
                                                &params, flags)
                   : rt_tile_stop_select_frames_async(ctx_, tiles_mean_max, tile_frames, stop_io, n_frames, stats_out, width,
                                                      height, &params, flags, nullptr),
              "tileStopSelectFrames");
    }

    rt_counters counters() const
    {
        rt_counters c;
        check(rt_get_counters(ctx_, &c), "counters");
        return c;
    }
    rt_ctx *handle() { return ctx_; }

private:
    void check(int st, const char *what) const
    {
        if (st != RT_OK)
            throw std::runtime_error(std::string(what) + ": " + rt_status_string(st) + " (" +
                                     (ctx_ ? rt_last_error(ctx_) : "") + ")");
    }
    rt_ctx *ctx_ = nullptr;
    std::vector<rt_sphere> spheres_;
    bool dirty_ = true;
    float fov_ = 53.0f;
    unsigned sampleRate_ = 8, maxPathDepth_ = 4;
};

#endif /* RAYTRACER_HIP_HPP */
