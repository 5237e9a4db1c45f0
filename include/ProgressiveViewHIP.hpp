/*
 * ProgressiveViewHIP.hpp — the interactive display step above the path tracer
 * (SURVEY.md §8f item 3), windowing-system free.
 *
 * GlutCLWindow (clrt/GlutCLWindow.cpp:136-301) owns the progressive-refinement loop,
 * the camera controls and the readback into the pixel buffer object it draws.  This
 * class is that state machine with the GL calls left to the host toolkit:
 *
 *   display()        glutDisplayCallback (:136-188): after a (re)allocation render with
 *                    progression 0, else refine while progression < maxProgression
 *                    (progression++), then the non-sharing readback (:214-225) into
 *                    pixels(); returns true when another redisplay should be posted
 *                    (glutPostRedisplay, :149-150, :157); rendered() tells whether it traced;
 *   reshape(w, h)    glutReshapeCallback (:113-134): new buffer at the next display;
 *   specialKey(k)    glutSpecialKeypressCallback (:228-262): arrows orbit the camera by
 *                    3 degrees (azimuth mod 360, elevation clamped to [10, 90]) about
 *                    (0, -4, 0), then restart();
 *   motion(dx, dy)   glutMotionCallback (:270-281): drag orbits by (dx, dy) degrees;
 *   restart()        (:294-301): progression back to 0.  Returns true when a redisplay must
 *                    be posted: refinement had finished (progression >= maxProgression), so
 *                    no display is pending — without it the window would stay frozen on the
 *                    old view.  specialKey and motion return restart()'s answer.
 *
 * The orbit state starts at GlutCLWindow's constructor values (azimuth 105, elevation
 * 40, distance 5, :24-28), independent of the camera the application set — as in the
 * reference.  A GLUT (or any toolkit) window forwards its callbacks here and draws
 * pixels() (RGBA32F, W*H*4, bottom row first as glDrawPixels expects: the tracer's row 0).
 *
 *   setDenoise(on, params)   (no counterpart in the reference) display the edge-avoiding a-trous
 *                    filter of the frame instead of the raw Monte-Carlo frame: every traced
 *                    display still renders into the accumulation buffer, which the filter only
 *                    reads — the progressive result stays the reference's bit for bit — then
 *                    filters it on the GPU into a second device buffer, guided by the first-hit
 *                    features (rendered only after a reallocation or a camera change), and reads
 *                    that one back into pixels().  rawPixels() fetches the undenoised frame on
 *                    request.  Off (the default), every call does exactly what it did before.
 *   setTemporal(on, params)  (no counterpart in the reference) carry the displayed frame across
 *                    camera moves: the view keeps the last displayed (merged)
 *                    frame with its per-pixel history length, features and camera; at the first
 *                    display after a key press, a drag or a restart it reprojects them into the new
 *                    view, and every display shows the blend of that carried history with the
 *                    accumulation buffer (then filtered, with the denoiser on).  The accumulation
 *                    buffer is only read; rawPixels() returns it.  The history is dropped at a
 *                    reshape; the scene is assumed static.  Off (the default), nothing changes.
 *   setVarianceGuided(on, params)  (no counterpart in the reference) display the variance-guided
 *                    filter in place of setDenoise's: the view copies the
 *                    accumulation buffer on the device before every render that refines it, folds
 *                    the frame's luminance into its moments after the render, estimates the variance
 *                    of the frame about to be displayed (the accumulation buffer with the history
 *                    length n everywhere, or with setTemporal the merged frame, whose moments are
 *                    reprojected and merged next to the colour, with the merged lengths) and shows
 *                    rt_denoise_var's output.  Features are rendered as with setDenoise; rawPixels()
 *                    is unchanged; a reshape drops the moments.  Switched on in mid-accumulation,
 *                    the moments start from the accumulated frame.  Off (the default), nothing changes.
 *   setMotionCarry(on, max_history)  (no counterpart in the reference) with setTemporal, carry the
 *                    displayed frame (and setVarianceGuided's moments) across updateMesh as well
 *                    (DESIGN.md §4.13): the view keeps the pose the last frame was displayed in, and the
 *                    first display after the update reprojects the history through the new features
 *                    warped into that pose (rt_warp_features), its length capped at max_history.  The
 *                    denoisers read the unwarped features.  Off (the default), updateMesh drops the
 *                    history as before.
 *   setHistoryTrust(on, params)  (no counterpart in the reference) with setTemporal, judge the carried
 *                    history afresh at every display: rt_history_trust tests it against
 *                    the accumulation buffer over each pixel's window and gives the length it still
 *                    deserves, which both merges (colour and moments) take in place of the carried
 *                    length.  The carried pair itself is not rewritten.  Off (the default), no call is
 *                    made and no output bit changes.
 *   sceneChanged()   (no counterpart in the reference) the caller has changed the spheres (addSphere /
 *                    clearSpheres — the lights of RT_KERNEL_TRIS among them): the features are rendered
 *                    again and the progression restarts.  The history and the moments are dropped, as
 *                    updateMesh drops them without the motion carry — unless setHistoryTrust is on, which
 *                    keeps them and lets the test shorten them where the shading has changed.
 *   setSphereCarry(on, max_history)  (no counterpart in the reference) with setTemporal, in a view of a sphere
 *                    kernel, carry the displayed frame (and setVarianceGuided's moments) across sceneChanged()
 *                    (DESIGN.md §4.16): the view keeps the sphere list every frame was displayed with, and the
 *                    first display after the change reprojects the history through the new features with
 *                    every sphere pixel put back where its sphere stood (rt_warp_features_spheres), its length
 *                    capped at max_history.  The caller's contract: sphere i before and after the change is
 *                    the same object — a caller who reorders the list leaves the carry off for that change.
 *                    The denoisers and setHistoryTrust read the unwarped features; with setHistoryTrust both
 *                    apply: the warp puts the history on the sphere, the test shortens it where shadows and
 *                    reflections changed.  In an RT_KERNEL_TRIS view (its spheres are lights only: no pixel
 *                    carries a sphere id) and off (the default), sceneChanged() does what it did before: no
 *                    call is made, nothing is allocated, no output bit changes.
 *   setToneMap(on, params, autoExposure, meter)  (no counterpart in the reference) the last display stage
 *                    (DESIGN.md §4.15): whatever the stages above chose to show is metered (with
 *                    autoExposure: the exposure is a float on the device that the meter reads and writes at
 *                    every traced display, so `meter.rate` < 1 adapts smoothly; without it params.exposure
 *                    holds) and tone-mapped into an RGBA8 device buffer, which display() reads back into
 *                    pixels8() (W*H words r | g << 8 | b << 16 | 255 << 24, bottom row first as
 *                    glDrawPixels(GL_RGBA, GL_UNSIGNED_BYTE) expects).  The shown float frame is only read:
 *                    pixels() is what it was without the stage.  The exposure starts afresh ("none") at a
 *                    (re)allocation and when the stage is switched on; restart(), updateMesh() and
 *                    sceneChanged() keep it.  Off (the default), nothing changes, allocation included.
 *   setConverge(on, params, minFrames)  (no counterpart in the reference) refine until converged (DESIGN.md
 *                    §4.17): every traced display meters what the stages above chose to show, before any
 *                    filter — the accumulation buffer, or with setTemporal the merged history — against the
 *                    variance of its luminance (rt_variance, from the view's moments, which are then kept
 *                    whether setVarianceGuided is on or not) with rt_noise_meter, and reads the sixteen
 *                    bytes of stats back with the frame.  Once at least minFrames frames are in the view's
 *                    moments, a pixel was counted and the level is at or under params.threshold, the view
 *                    is converged(): that display() returns false and later ones trace nothing, until
 *                    restart(), a key, a drag, a reshape, updateMesh or sceneChanged() — which then ask for
 *                    a redisplay as they do after maxProgression.  What is displayed does not change.  Off
 *                    (the default), nothing changes, allocation included.
 *   setAdaptive(on, params)  (no counterpart in the reference) with setConverge, in a view of RT_KERNEL_TRIS without
 *                    setTemporal (or with it and setAdaptiveHistory, below): stop tracing the 8x8 tiles the noise meter calls quiet.  The
 *                    view keeps a stop plane on the device (a word per tile: 0 = refined, k = stopped after k
 *                    frames) that masks its renders (rt_set_tile_stop); the moments and the history lengths
 *                    follow it (rt_moments_accumulate_tiles), the meter's tile map is always computed, and once
 *                    the view's moments hold setConverge's minFrames frames rt_tile_stop_select updates the plane
 *                    on the device after every traced display.  A stopped tile keeps its pixels and stays
 *                    stopped until the plane is zeroed: at a (re)allocation, a key, a drag, restart(),
 *                    updateMesh and sceneChanged().  The view is converged() by setConverge's rule, or when no
 *                    tile is live.  In any other view (adaptiveInEffect() false) and off (the default), nothing
 *                    changes and no plane is set.
 *   setSampleBudget(on, params)  (no counterpart in the reference) where setAdaptive is in effect: give the noisy tiles
 *                    extra passes per display.  It takes effect at the next display at which the
 *                    frame count starts afresh (after a (re)allocation, a key, a drag, restart(), updateMesh,
 *                    sceneChanged()), where the view zeroes a count plane beside the stop plane.  A display of
 *                    progression 0 is rendered as ever; every later one renders each pass at progression 0 into a
 *                    scratch frame under the pass's mask (rt_tile_pass_mask) and folds it into the accumulation
 *                    buffer with the weight the tile's own count gives (rt_fold_tiles), which also keeps the
 *                    moments and the history lengths; after the stop rule rt_tile_budget sets every tile's passes
 *                    for the next display from the same tile map.  With max_passes 1 every byte displayed is the
 *                    one setAdaptive alone displays.  Until it takes effect, where setAdaptive is not in effect
 *                    and off (the default), every byte and every call is what it was.
 *   setAdaptiveHistory(on)  (no counterpart in the reference) lets setAdaptive (and with it setSampleBudget) take effect
 *                    in a view with setTemporal too.  The stop plane, the masked renders, the
 *                    moments, the pass loop and the fold run as they do without setTemporal; both merges (colour and
 *                    moments) and setHistoryTrust's test take the accumulation buffer's frame count per pixel, from
 *                    the plane of lengths the masked moments and the fold keep (rt_temporal_merge_len,
 *                    rt_history_trust_len), so the kept lengths are min(own count + carried length, max_history) per
 *                    pixel and a stopped tile's merged pixels stop changing.  After the meter rt_tile_len_min takes
 *                    every tile's shortest kept length among its surface pixels, and the stop rule runs at every
 *                    traced display through rt_tile_stop_select_frames: a tile can stop once that length reaches
 *                    min(params.min_frames, max_history), whatever the view's own frame count — after a move, a tile
 *                    that long, quiet history covers stops at once, and the passes go to the disoccluded ones.
 *                    setConverge's minFrames gates the frame-wide rule alone.  The planes are zeroed where setAdaptive
 *                    zeroes them; the history survives those events as setTemporal, the carries and setHistoryTrust
 *                    decide.  Off (the default), every byte and every call is what it was: setAdaptive is not in
 *                    effect with setTemporal.
 *   setFloatReadback(on)  with setToneMap: off, display() reads back only the 8-bit frame (a quarter of
 *                    the bytes) and pixels() keeps its last contents — those of the last display with the
 *                    readback on, zeros before any; rawPixels() still fetches the accumulation buffer.  On
 *                    (the default), and always without setToneMap, pixels() is read at every display.
 */
#ifndef PROGRESSIVE_VIEW_HIP_HPP
#define PROGRESSIVE_VIEW_HIP_HPP

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "RayTracerHIP.hpp"

class ProgressiveViewHIP {
public:
    enum Key { KEY_LEFT, KEY_RIGHT, KEY_UP, KEY_DOWN };

    ProgressiveViewHIP(RayTracerHIP &rt, unsigned width, unsigned height, int kernel = RT_KERNEL_SPHERES)
        : rt_(rt), width_(width), height_(height), kernel_(kernel), buf_(new Buffers)
    {
    }
    ~ProgressiveViewHIP()
    {
        if (plane_) rt_set_tile_stop(rt_.handle(), nullptr, 0, 0, 0); /* the tracer outlives the view's plane */
    }
    ProgressiveViewHIP(const ProgressiveViewHIP &) = delete;
    ProgressiveViewHIP &operator=(const ProgressiveViewHIP &) = delete;

    void setProgressive(unsigned maxProgression) { maxProgression_ = maxProgression; } /* GlutCLWindow.h */

    bool display()
    {
        bool again = false;
        rendered_ = false;
        if (realloc_) {
            allocate();
            progression_ = 0;
            trace();
            realloc_ = false;
            again = maxProgression_ > 0 && !converged_;
        } else if (progression_ < maxProgression_ && !converged_) {
            ++progression_;
            trace();
            again = !converged_; /* the display that converges posts no redisplay */
        }
        return again;
    }

    void reshape(unsigned w, unsigned h)
    {
        width_ = w;
        height_ = h;
        realloc_ = true;
    }

    bool specialKey(Key k)
    {
        switch (k) {
        case KEY_LEFT: azimuth_ = std::fmod(azimuth_ + 3.0f, 360.0f); break;
        case KEY_RIGHT: azimuth_ = std::fmod(azimuth_ - 3.0f, 360.0f); break;
        case KEY_UP: elevation_ = std::fmin(elevation_ + 3.0f, 90.0f); break;
        case KEY_DOWN: elevation_ = std::fmax(elevation_ - 3.0f, 10.0f); break;
        }
        orbit();
        return restart();
    }

    bool motion(int dx, int dy)
    {
        azimuth_ = std::fmod(azimuth_ + (float)dx, 360.0f);
        elevation_ = std::fmax(std::fmin(elevation_ + (float)dy, 90.0f), 10.0f);
        orbit();
        return restart();
    }

    bool restart()
    {
        const bool post = progression_ >= maxProgression_ || converged_;
        converged_ = false;
        progression_ = 0;
        carry_ = true;
        stopReset_ = true; /* setAdaptive: every tile is live again */
        return post;
    }

    /* The mesh moves (RayTracerHIP::updateMesh): the features are rendered again, and what the
       display stages keep of earlier frames — the temporal history and the luminance moments —
       is dropped, not carried: it shows the old geometry.  With setMotionCarry (and setTemporal, and
       a kept frame) it is carried instead: the pose the kept frame was displayed in is snapshotted
       before the tracer is updated — only if no snapshot is pending, so several updates between two
       displays keep the oldest — and the next display warps its features into that pose
       (mergeTemporal).  Progression back to 0; returns restart()'s answer. */
    bool updateMesh(const float *verts_xyz, uint32_t n_verts, int flags = 0)
    {
        const bool carryMotion = motionCarry_ && temporal_ && haveHist_ && !realloc_;
        Buffers &b = *buf_;
        if (carryMotion && !(posePending_ && b.poseVerts == n_verts)) {
            if (b.poseVerts != n_verts) {
                b.posePrev.drop();
                b.poseVerts = n_verts;
            }
            b.posePrev.need((size_t)n_verts * 3, "pose snapshot");
            rt_.meshPose(b.posePrev.p, n_verts, true);
            posePending_ = true;
        }
        rt_.updateMesh(verts_xyz, n_verts, flags);
        featDirty_ = true;
        if (!carryMotion) dropHistory();
        const bool post = restart();
        if (!carryMotion) carry_ = false;
        return post;
    }
    /* (no counterpart in the reference) carry the displayed frame across updateMesh (DESIGN.md
       §4.13).  max_history caps the history length of that carry alone (with setTemporal's own cap):
       the carried radiance is the old pose's, and the cap bounds how long its shading lags.  Needs
       setTemporal; off (the default), updateMesh drops the history as before. */
    void setMotionCarry(bool on, float max_history = 8.0f)
    {
        motionCarry_ = on;
        motionMaxHistory_ = max_history;
        if (!on) posePending_ = false;
    }
    bool motionCarry() const { return motionCarry_; }

    /* (no counterpart in the reference) lag-adaptive trust of the carried history.
       Needs setTemporal; off (the default), nothing changes. */
    void setHistoryTrust(bool on, const rt_trust_params &params = RayTracerHIP::trustDefaults())
    {
        trust_ = on;
        trustParams_ = params;
    }
    bool historyTrust() const { return trust_; }
    /* (no counterpart in the reference) carry the displayed frame across sceneChanged() in a view of a
       sphere kernel.  max_history caps the history length of that carry alone (with
       setTemporal's own cap): reflections and refractions in a moved sphere lag, and the cap bounds for
       how long.  Sphere i before and after a change must be the same object; a caller who reorders the
       list leaves the carry off for that change.  Needs setTemporal; off (the default), sceneChanged()
       does what it did before. */
    void setSphereCarry(bool on, float max_history = 8.0f)
    {
        sphereCarry_ = on;
        sphereMaxHistory_ = max_history;
        if (!on) {
            spheresPending_ = shownValid_ = false;
            shownSpheres_.clear();
        }
    }
    bool sphereCarry() const { return sphereCarry_; }
    /* The spheres have changed (the caller's addSphere / clearSpheres).  Without setHistoryTrust the
       history and the moments show the old lighting and are dropped; with it they are kept and judged.
       With setSphereCarry (and setTemporal, a sphere kernel and a kept frame) they are kept too, and the
       next display seeks every sphere pixel's history where its sphere stood when the kept frame was
       displayed (mergeTemporal) — several changes between two displays keep that oldest list, which is
       copied at displays only.  Progression back to 0; returns restart()'s answer. */
    bool sceneChanged()
    {
        const bool carrySpheres =
            sphereCarry_ && temporal_ && haveHist_ && shownValid_ && !realloc_ && kernel_ != RT_KERNEL_TRIS;
        featDirty_ = true;
        if (carrySpheres) spheresPending_ = true;
        else if (!trust_) dropHistory();
        const bool post = restart();
        if (!carrySpheres && !trust_) carry_ = false;
        return post;
    }

    void setDenoise(bool on, const rt_denoise_params &params = RayTracerHIP::denoiseDefaults())
    {
        if (on && !denoise_) featDirty_ = true;
        denoise_ = on;
        denoiseParams_ = params;
    }
    bool denoising() const { return denoise_; }
    void setTemporal(bool on, const rt_reproject_params &params = RayTracerHIP::reprojectDefaults())
    {
        if (on && !temporal_) {
            featDirty_ = true;
            dropHistory(false); /* the moments follow the accumulation buffer, not the display */
        }
        temporal_ = on;
        temporalParams_ = params;
    }
    bool temporal() const { return temporal_; }
    void setVarianceGuided(bool on, const rt_denoise_var_params &params = RayTracerHIP::denoiseVarDefaults())
    {
        if (on && !varGuided_) {
            featDirty_ = true;
            dropHistory();
        }
        varGuided_ = on;
        varParams_ = params;
    }
    bool varianceGuided() const { return varGuided_; }
    /* (no counterpart in the reference) refine until converged: see the file comment */
    void setConverge(bool on, const rt_noise_params &params = RayTracerHIP::noiseDefaults(), unsigned minFrames = 8)
    {
        if (on && !momentsWanted()) { /* no moments are kept: as setVarianceGuided(true) from off */
            featDirty_ = true;
            dropHistory();
        }
        converge_ = on;
        convergeParams_ = params;
        convergeMinFrames_ = minFrames;
        converged_ = false; /* the next traced display decides afresh */
    }
    /* whether the last traced display found the view converged: display() traces no more until a
       restart(), a reallocation, updateMesh or sceneChanged */
    bool converged() const { return converged_; }
    /* the noise meter's figures of the last traced display with setConverge on (zeros before one) */
    const rt_noise_stats &noiseStats() const { return noiseStats_; }
    /* With setConverge: also compute the per-tile noise map at every traced display and read it back
       into noiseMap(): ceil(W/8) ceil(H/8) pairs (mean, max), row-major, bottom tile row first. */
    void setNoiseMapReadback(bool on) { noiseMapReadback_ = on; }
    const std::vector<float> &noiseMap() const { return noiseMap_; }

    /* (no counterpart in the reference) adaptive sampling on the meter's tile map: see the
       file comment.  params.min_frames holds beside setConverge's minFrames: no tile stops before both. */
    void setAdaptive(bool on, const rt_adaptive_params &params = RayTracerHIP::adaptiveDefaults())
    {
        if (on != adaptive_) stopReset_ = true;
        adaptive_ = on;
        adaptiveParams_ = params;
        converged_ = false; /* the next traced display decides afresh */
    }
    bool adaptiveInEffect() const { return adaptive_ && converge_ && kernel_ == RT_KERNEL_TRIS && (!temporal_ || adaptHistory_); }
    /* (no counterpart in the reference) setAdaptive under setTemporal, by per-pixel frame counts: see
       the file comment.  In effect where setAdaptive, setConverge, setTemporal and this are all on, in a view of
       RT_KERNEL_TRIS. */
    void setAdaptiveHistory(bool on)
    {
        if (on != adaptHistory_) stopReset_ = true;
        adaptHistory_ = on;
        converged_ = false; /* the next traced display decides afresh */
    }
    bool adaptiveHistoryInEffect() const { return adaptiveInEffect() && temporal_; }
    /* With setTemporal: also read the colour history's kept lengths back at every traced display into
       historyLengths(): W*H floats, bottom row first. */
    void setHistoryLengthReadback(bool on) { histLenReadback_ = on; }
    const std::vector<float> &historyLengths() const { return histLen_; }
    /* the stop rule's figures after the last traced display with setAdaptive in effect (zeros before one) */
    const rt_adaptive_stats &adaptiveStats() const { return adaptiveStats_; }
    /* With setAdaptive in effect: also read the stop plane back at every traced display into stopMap():
       ceil(W/8) ceil(H/8) words, row-major, bottom tile row first. */
    void setStopMapReadback(bool on) { stopMapReadback_ = on; }
    const std::vector<uint32_t> &stopMap() const { return stopMap_; }

    /* (no counterpart in the reference) per-tile sample counts: see the file comment.  In effect
       only where setAdaptive is, and from the next display at which the frame count starts afresh. */
    void setSampleBudget(bool on, const rt_budget_params &params = RayTracerHIP::budgetDefaults())
    {
        budget_ = on;
        budgetParams_ = params;
    }
    /* whether the last traced display ran (or, at progression 0, began) the pass loop */
    bool sampleBudgetInEffect() const { return budgetActive_; }
    /* the budget rule's figures after the last traced display that ran it (zeros before one): the passes of the next */
    const rt_budget_stats &budgetStats() const { return budgetStats_; }
    /* With setSampleBudget in effect: also read the count plane back at every traced display into sampleCounts():
       ceil(W/8) ceil(H/8) words, the frames folded into each tile's mean since progression 0's. */
    void setSampleCountReadback(bool on) { countReadback_ = on; }
    const std::vector<uint32_t> &sampleCounts() const { return sampleCounts_; }

    /* (no counterpart in the reference) the tone-mapped 8-bit display output */
    void setToneMap(bool on, const rt_tonemap_params &params = RayTracerHIP::toneMapDefaults(), bool autoExposure = true,
                    const rt_meter_params &meter = RayTracerHIP::meterDefaults())
    {
        if (on && !toneMap_) exposureReset_ = true;
        toneMap_ = on;
        toneParams_ = params;
        autoExposure_ = autoExposure;
        meterParams_ = meter;
    }
    bool toneMapping() const { return toneMap_; }
    void setFloatReadback(bool on) { floatReadback_ = on; }
    bool floatReadback() const { return floatReadback_; }
    /* The tone-mapped frame of the last traced display with setToneMap on (empty before one). */
    const std::vector<uint32_t> &pixels8() const { return pbo8_; }
    /* The exposure the last traced display was tone-mapped under: the metered one, read back now, or
       params.exposure without autoExposure; 0 before a display with setToneMap on. */
    float exposure() const
    {
        if (!toneMap_ || pbo8_.empty()) return 0.0f;
        if (!autoExposure_) return toneParams_.exposure;
        float e = 0.0f;
        if (!buf_->exposure.p || hipMemcpy(&e, buf_->exposure.p, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            throw std::runtime_error("ProgressiveViewHIP: exposure readback failed");
        return e;
    }

    /* With setToneMap and setFloatReadback(false): the contents of the last display that read it back. */
    const std::vector<float> &pixels() const { return pbo_; }
    /* The accumulation buffer as rendered (what pixels() holds with the denoiser off), read back now. */
    const std::vector<float> &rawPixels()
    {
        if (!denoise_ && !temporal_ && !varGuided_ && !(toneMap_ && !floatReadback_)) return pbo_;
        raw_.assign(pbo_.size(), 0.0f);
        const float *dev = buf_->dev.p;
        if (dev && hipMemcpy(raw_.data(), dev, raw_.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            throw std::runtime_error("ProgressiveViewHIP: raw frame readback failed");
        return raw_;
    }
    unsigned progression() const { return progression_; }
    unsigned maxProgression() const { return maxProgression_; }
    bool rendered() const { return rendered_; }
    float azimuth() const { return azimuth_; }
    float elevation() const { return elevation_; }
    float distance() const { return distance_; }
    unsigned width() const { return width_; }
    unsigned height() const { return height_; }

private:
    void orbit()
    {
        const float target[3] = {0.0f, -4.0f, 0.0f};
        rt_.setCameraSpherical(target, elevation_, azimuth_, distance_);
        featDirty_ = true;
    }
    /* device memory with one owner: allocated when first needed, freed when dropped or destroyed */
    struct DeviceFloats {
        float *p = nullptr;
        DeviceFloats() = default;
        DeviceFloats(const DeviceFloats &) = delete;
        DeviceFloats &operator=(const DeviceFloats &) = delete;
        ~DeviceFloats() { drop(); }
        void need(size_t floats, const char *what)
        {
            if (!p && hipMalloc(&p, floats * sizeof(float)) != hipSuccess)
                throw std::runtime_error(std::string("ProgressiveViewHIP: ") + what + " allocation failed");
        }
        void drop()
        {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
    };
    /* What setTemporal keeps of a displayed quantity: the merged frame of the last display, and the one
       carried into the current view, which every display of that view merges with.  Each is an RGBA
       frame followed by its plane of history lengths. */
    struct History {
        struct Pair {
            DeviceFloats buf;
            size_t px = 0;
            float *rgba() const { return buf.p; }
            float *len() const { return buf.p + 4 * px; }
        } kept, carried;
        void need(size_t pixels, const char *what)
        {
            kept.px = carried.px = pixels;
            kept.buf.need(5 * pixels, what);
            carried.buf.need(5 * pixels, what);
        }
    };
    /* everything the view holds on the device for one frame size: a reshape replaces the lot */
    struct Buffers {
        DeviceFloats dev;      /* the accumulation buffer the tracer renders into */
        DeviceFloats den;      /* setDenoise / setVarianceGuided: the filtered frame */
        DeviceFloats feat;     /* the view's first-hit features */
        DeviceFloats featPrev; /* setTemporal: the features the kept frame was displayed with */
        History colour;        /* setTemporal: the displayed frame */
        /* setMotionCarry: the pose the kept frame was displayed in (a device copy taken at the first
           updateMesh after a display), and the current features warped into it */
        DeviceFloats posePrev, featWarp;
        uint32_t poseVerts = 0;
        /* setSphereCarry: the spheres the kept frame was displayed with, uploaded for the warp (which
           shares featWarp) */
        DeviceFloats spherePrev;
        size_t spherePrevCount = 0;
        DeviceFloats trustLen; /* setHistoryTrust: the lengths the carried history still deserves at this display */
        /* setVarianceGuided: the accumulation buffer before the frame, the view's moments, with
           setTemporal their history, the variance plane and (without setTemporal) the plane of history lengths */
        DeviceFloats accPrev, mom, var, len;
        History moments;
        /* setToneMap: the RGBA8 frame (W*H words) and the metered exposure (one float; 0: none yet) */
        DeviceFloats tone8, exposure;
        /* setConverge: the meter's stats (four words) and, with setNoiseMapReadback, the tile pairs */
        DeviceFloats noiseStats, noiseTiles;
        /* setAdaptive: the stop plane (a word per tile) and the stop rule's stats (four words); the per-pixel
           history lengths are in `len` */
        DeviceFloats stop, adaptStats;
        DeviceFloats tileLen; /* setAdaptiveHistory: every tile's shortest kept history length (a float per tile) */
        /* setSampleBudget: the frame a pass is rendered into, the count, passes and mask planes (a word per tile)
           and the budget rule's stats */
        DeviceFloats sample, count, passes, mask, budgetStats;
    };
    /* setVarianceGuided or setConverge: the view keeps the accumulation copy, the moments and the variance plane */
    bool momentsWanted() const { return varGuided_ || converge_; }

    /* What earlier frames left is no longer valid: the next display starts the history afresh (and
       the moments, unless the caller keeps them). */
    void dropHistory(bool moments = true)
    {
        haveHist_ = false;
        posePending_ = false;
        spheresPending_ = false;
        if (moments) momValid_ = false;
        if (moments) stopReset_ = true; /* the moments start afresh: so do the tiles */
    }
    void allocate()
    {
        clearPlane(); /* (the tracer borrows the old size's plane) */
        buf_.reset(new Buffers); /* frees the old size's buffers, the pose snapshot among them */
        buf_->dev.need((size_t)width_ * height_ * 4, "framebuffer");
        pbo_.assign((size_t)width_ * height_ * 4, 0.0f);
        pbo8_.clear();
        noiseMap_.clear();
        noiseStats_ = rt_noise_stats{};
        adaptiveStats_ = rt_adaptive_stats{};
        budgetStats_ = rt_budget_stats{};
        budgetActive_ = haveBudget_ = false;
        sampleCounts_.clear();
        stopMap_.clear();
        histLen_.clear();
        stopReset_ = true;
        converged_ = false;
        frames_ = 0;
        exposureReset_ = true;
        featDirty_ = true;
        dropHistory();
    }
    /* The view's features, rendered again where a camera move, a mesh or scene change or a setter has
       made them stale.  Returns the features the kept frame was displayed with: with setTemporal a
       re-render keeps the previous ones (the swap) and makes this display carry the history. */
    const float *refreshFeatures()
    {
        Buffers &b = *buf_;
        const size_t floats = (size_t)width_ * height_ * 8;
        b.feat.need(floats, "feature buffer");
        if (temporal_) b.featPrev.need(floats, "feature buffer");
        if (!featDirty_) return b.feat.p;
        if (temporal_) {
            std::swap(b.feat.p, b.featPrev.p);
            carry_ = true;
        }
        rt_.renderFeatures(b.feat.p, width_, height_, kernel_, true);
        featDirty_ = false;
        return temporal_ ? b.featPrev.p : b.feat.p;
    }
    /* The merged frame of this display into the colour history's kept pair; with kept moments (setVarianceGuided,
       setConverge) the view's moments go the same way into theirs.  Both take their lengths from the colour history:
       they keep one length.  The accumulation buffer's frame count is n, or with curLen (setAdaptiveHistory in effect)
       each pixel's own of that plane. */
    void mergeTemporal(const float *histFeat, float n, const float *curLen)
    {
        Buffers &b = *buf_;
        const size_t px = (size_t)width_ * height_;
        b.colour.need(px, "history buffer");
        if (momentsWanted()) b.moments.need(px, "moments history buffer");
        const History *const hist[] = {&b.colour, &b.moments}; /* the active ones, and what this display merges into each */
        const float *const cur[] = {b.dev.p, b.mom.p};
        const int nHist = momentsWanted() ? 2 : 1;
        const rt_camera cam = rt_.getCamera(width_);
        const bool judged = trust_ && haveHist_; /* a history exists: it is judged at every display */
        if (!haveHist_) { /* after a (re)allocation or a drop: no history anywhere */
            bool ok = true;
            for (int i = 0; i < nHist; ++i) ok = ok && hipMemset(hist[i]->carried.rgba(), 0, 5 * px * sizeof(float)) == hipSuccess;
            if (!ok || hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("ProgressiveViewHIP: history reset failed");
        } else if (carry_) { /* a new accumulation begins: carry the kept frames into it */
            const float *curFeat = b.feat.p;
            rt_reproject_params prm = temporalParams_;
            if (posePending_) { /* the mesh has moved since: the taps are sought where the material was */
                b.featWarp.need(8 * px, "feature buffer");
                rt_.warpFeatures(b.feat.p, b.posePrev.p, b.poseVerts, b.featWarp.p, width_, height_, true);
                curFeat = b.featWarp.p;
                prm.max_history = std::fmin(temporalParams_.max_history, motionMaxHistory_);
            }
            if (spheresPending_) { /* spheres have moved since: the taps are sought where each sphere stood */
                const size_t n = shownSpheres_.size();
                if (b.spherePrevCount != n) {
                    b.spherePrev.drop();
                    b.spherePrevCount = n;
                }
                if (n) {
                    b.spherePrev.need(n * (sizeof(rt_sphere) / sizeof(float)), "sphere list");
                    if (hipMemcpy(b.spherePrev.p, shownSpheres_.data(), n * sizeof(rt_sphere), hipMemcpyHostToDevice) != hipSuccess)
                        throw std::runtime_error("ProgressiveViewHIP: sphere list upload failed");
                }
                b.featWarp.need(8 * px, "feature buffer");
                rt_.warpFeaturesSpheres(curFeat, reinterpret_cast<const rt_sphere *>(b.spherePrev.p), (uint32_t)n, b.featWarp.p,
                                        width_, height_, true);
                curFeat = b.featWarp.p;
                prm.max_history = std::fmin(prm.max_history, sphereMaxHistory_);
            }
            for (int i = 0; i < nHist; ++i) /* the same lengths, features and cameras: the same taps and weights */
                rt_.reproject(hist[i]->kept.rgba(), b.colour.kept.len(), histFeat, histCam_, curFeat, hist[i]->carried.rgba(),
                              hist[i]->carried.len(), width_, height_, prm, true);
        }
        posePending_ = false;
        spheresPending_ = false;
        carry_ = false;
        /* the lengths the merges blend by: the carried ones, or with setHistoryTrust what this display's
           accumulation buffer leaves of the colour's (one plane for both) */
        if (judged) {
            b.trustLen.need(px, "trusted history length buffer");
            if (curLen)
                rt_.historyTrustLen(b.colour.carried.rgba(), b.colour.carried.len(), b.dev.p, curLen, b.feat.p, b.trustLen.p, width_,
                                    height_, trustParams_, true);
            else
                rt_.historyTrust(b.colour.carried.rgba(), b.colour.carried.len(), b.dev.p, n, b.feat.p, b.trustLen.p, width_, height_,
                                 trustParams_, true);
        }
        for (int i = 0; i < nHist; ++i) {
            const float *histLen = judged ? b.trustLen.p : hist[i]->carried.len();
            if (curLen)
                rt_.temporalMergeLen(hist[i]->carried.rgba(), histLen, cur[i], curLen, temporalParams_.max_history,
                                     hist[i]->kept.rgba(), hist[i]->kept.len(), width_, height_, true);
            else
                rt_.temporalMerge(hist[i]->carried.rgba(), histLen, cur[i], n, temporalParams_.max_history, hist[i]->kept.rgba(),
                                  hist[i]->kept.len(), width_, height_, true);
        }
        histCam_ = cam;
        haveHist_ = true;
    }
    /* before a render that refines the accumulation buffer: its copy, for the frame's own sample */
    void keepAccumulation()
    {
        Buffers &b = *buf_;
        const size_t frame = (size_t)width_ * height_ * 4;
        b.accPrev.need(frame, "accumulation copy");
        if (progression_ > 1 && (hipMemcpy(b.accPrev.p, b.dev.p, frame * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess ||
                                 hipDeviceSynchronize() != hipSuccess))
            throw std::runtime_error("ProgressiveViewHIP: accumulation copy failed");
    }
    /* kept moments without setTemporal: one view, n frames everywhere */
    const float *constantLengths(float n)
    {
        const size_t px = (size_t)width_ * height_;
        buf_->len.need(px, "history length buffer");
        const std::vector<float> lens(px, n);
        if (hipMemcpy(buf_->len.p, lens.data(), px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("ProgressiveViewHIP: history length upload failed");
        return buf_->len.p;
    }
    /* setToneMap: meter what is shown (the exposure float stays on the device: no host sync between the
       meter and the tone map), then tone-map it into the 8-bit buffer. */
    void toneMapShown(const float *shown)
    {
        Buffers &b = *buf_;
        b.tone8.need((size_t)width_ * height_, "8-bit framebuffer");
        const float *exposure = nullptr;
        if (autoExposure_) {
            if (!b.exposure.p) exposureReset_ = true; /* (a new float holds nothing yet) */
            b.exposure.need(1, "exposure");
            if (exposureReset_ && (hipMemset(b.exposure.p, 0, sizeof(float)) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
                throw std::runtime_error("ProgressiveViewHIP: exposure reset failed");
            exposureReset_ = false;
            rt_.meterExposure(shown, b.exposure.p, nullptr, width_, height_, meterParams_, true, /*sync=*/false);
            exposure = b.exposure.p;
        }
        rt_.toneMap(shown, exposure, reinterpret_cast<uint32_t *>(b.tone8.p), width_, height_, toneParams_, true);
    }
    size_t noiseTileCount() const { return (size_t)((width_ + 7u) / 8u) * ((height_ + 7u) / 8u); }
    /* setConverge: meter what stage (6) chose to show, before any filter, with the variance plane just
       estimated for it; the stats (and with setNoiseMapReadback the tile pairs) stay on the device
       until the frame's readback. */
    void meterShown(const float *shown, bool sync, bool tiles)
    {
        Buffers &b = *buf_;
        b.noiseStats.need(sizeof(rt_noise_stats) / sizeof(float), "noise stats");
        if (tiles) b.noiseTiles.need(2 * noiseTileCount(), "noise tile map");
        rt_.noiseMeter(shown, b.var.p, reinterpret_cast<rt_noise_stats *>(b.noiseStats.p), tiles ? b.noiseTiles.p : nullptr,
                       nullptr, width_, height_, convergeParams_, true, sync);
    }
    /* setAdaptive: the tracer's renders are whole frames again */
    void clearPlane()
    {
        if (plane_) rt_.setTileStop(nullptr);
        plane_ = nullptr;
    }
    /* the plane the tracer borrows: the stop plane, or in the pass loop the mask of the pass */
    void borrowPlane(const float *plane)
    {
        if (plane_ != plane) rt_.setTileStop(reinterpret_cast<const uint32_t *>(plane), width_, height_, true);
        plane_ = plane;
    }
    /* setAdaptive in effect: the view's plane, zeroed where the accumulation starts afresh, masks the renders */
    void maskRenders()
    {
        Buffers &b = *buf_;
        b.stop.need(noiseTileCount(), "stop plane");
        b.adaptStats.need(sizeof(rt_adaptive_stats) / sizeof(float), "stop rule stats");
        if (budgetActive_) {
            b.sample.need((size_t)width_ * height_ * 4, "sample frame");
            b.count.need(noiseTileCount(), "count plane");
            b.passes.need(noiseTileCount(), "passes plane");
            b.mask.need(noiseTileCount(), "pass mask");
            b.budgetStats.need(sizeof(rt_budget_stats) / sizeof(float), "budget stats");
        }
        /* (the counts start with the stop plane; until a budget says otherwise every tile has one pass) */
        if (stopReset_ && budgetActive_ &&
            (hipMemset(b.count.p, 0, noiseTileCount() * sizeof(uint32_t)) != hipSuccess ||
             hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b.passes.p), 1, noiseTileCount()) != hipSuccess))
            throw std::runtime_error("ProgressiveViewHIP: count plane reset failed");
        if (stopReset_) {
            budgetStats_ = rt_budget_stats{};
            haveBudget_ = false;
        }
        if (stopReset_ && (hipMemset(b.stop.p, 0, noiseTileCount() * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
            throw std::runtime_error("ProgressiveViewHIP: stop plane reset failed");
        stopReset_ = false;
        borrowPlane(b.stop.p);
    }
    /* setSampleBudget in effect, after progression 0: every pass of this display — its mask, a masked render at
       progression 0 into the scratch frame (which overwrites the live tiles' pixels with the frame's own sample), and
       the fold of those tiles into the accumulation buffer by their own counts, with the moments and the lengths.
       All passes but the last are enqueued without a wait. */
    void tracePasses()
    {
        Buffers &b = *buf_;
        const size_t px = (size_t)width_ * height_;
        b.mom.need(4 * px, "moments buffer");
        b.len.need(px, "history length buffer");
        const uint32_t *stop = reinterpret_cast<const uint32_t *>(b.stop.p), *passes = reinterpret_cast<const uint32_t *>(b.passes.p);
        const uint32_t rounds = haveBudget_ ? budgetStats_.rounds : 1u;
        borrowPlane(b.mask.p);
        rt_.flushScene();
        for (uint32_t r = 0; r < rounds; ++r) {
            rt_.tilePassMask(stop, passes, r, reinterpret_cast<uint32_t *>(b.mask.p), width_, height_, true, /*sync=*/false);
            if (r + 1 < rounds) {
                if (rt_render_async(rt_.handle(), b.sample.p, width_, height_, 0, kernel_, nullptr, RT_OUT_DEVICE, nullptr) != RT_OK)
                    throw std::runtime_error(std::string("ProgressiveViewHIP: pass render failed: ") + rt_last_error(rt_.handle()));
            } else
                rt_.rayTrace(b.sample.p, width_, height_, 0, kernel_, true);
            rt_.foldTiles(b.sample.p, b.dev.p, reinterpret_cast<uint32_t *>(b.count.p), passes, r, b.mom.p, b.mom.p, b.len.p, width_,
                          height_, true, /*sync=*/false);
        }
        borrowPlane(b.stop.p);
    }
    /* One traced display, whatever is switched on: render, then compose what is shown from the
       accumulation buffer, which every stage only reads. */
    void trace()
    {
        Buffers &b = *buf_;
        const size_t px = (size_t)width_ * height_;
        const float n = (float)(progression_ > 1 ? progression_ : 1);
        const bool adapt = adaptiveInEffect();
        const bool adaptHist = adapt && temporal_; /* setAdaptiveHistory in effect: the frame counts are b.len's */
        /* setSampleBudget begins where the frame count starts afresh — the planes are zeroed (restart() and allocate()
           ask for it) before progression 0, or before progression 1, the first display after a restart(), whose
           weight is 1 — and ends with what it depends on, or where the planes are zeroed in mid-accumulation */
        if (!budget_ || !adapt || (stopReset_ && progression_ > 1)) budgetActive_ = false;
        else if (stopReset_) budgetActive_ = true;
        const bool passes = budgetActive_ && progression_ > 0; /* (the fold reads the old frame itself: no copy) */
        if (momentsWanted() && !passes) keepAccumulation();
        if (adapt) maskRenders();
        else {
            clearPlane();
            stopReset_ = true; /* (in effect again later: from a zero plane) */
        }
        if (passes) {
            tracePasses();
            frames_ = n == 1.0f ? 1u : frames_ + 1u;
        } else
            rt_.rayTrace(b.dev.p, width_, height_, progression_, kernel_, true);
        if (momentsWanted() && !passes) {
            b.mom.need(4 * px, "moments buffer");
            /* (without valid moments, after it was switched on in mid-accumulation: start from this frame) */
            const float nMom = momValid_ ? n : 1.0f;
            if (adapt) { /* a stopped tile keeps its moments, and its pixels the length it stopped at */
                b.len.need(px, "history length buffer");
                rt_.momentsAccumulateTiles(b.accPrev.p, b.dev.p, nMom, b.mom.p, b.mom.p, reinterpret_cast<const uint32_t *>(b.stop.p),
                                           b.len.p, width_, height_, true);
            } else
                rt_.momentsAccumulate(b.accPrev.p, b.dev.p, nMom, b.mom.p, b.mom.p, width_, height_, true);
            momValid_ = true;
            frames_ = nMom == 1.0f ? 1u : frames_ + 1u; /* the frames in the view's own moments */
        }
        const float *histFeat = momentsWanted() || denoise_ || temporal_ ? refreshFeatures() : nullptr;
        /* what is displayed, its moments and its history lengths */
        const float *shown = b.dev.p, *moments = b.mom.p, *len = nullptr;
        if (temporal_) {
            mergeTemporal(histFeat, n, adaptHist ? b.len.p : nullptr);
            shown = b.colour.kept.rgba();
            moments = b.moments.kept.rgba();
            len = b.colour.kept.len();
        } else if (momentsWanted()) {
            len = adapt ? b.len.p : constantLengths(n);
        }
        if (varGuided_ || denoise_) b.den.need(4 * px, "denoised framebuffer");
        if (momentsWanted()) {
            b.var.need(px, "variance buffer");
            rt_.variance(shown, moments, len, b.feat.p, b.var.p, width_, height_, varParams_, true);
        }
        /* (the last of these calls waits for the stream, unless a filter's call does) */
        /* (with setAdaptiveHistory at every display: the gate is each tile's own, by its shortest merged history) */
        const bool select = adapt && (adaptHist || frames_ >= convergeMinFrames_);
        /* the budget rule follows every fold, and a stop rule that ran at progression 0 (minFrames <= 1): the fold
           goes by the passes plane alone, where a stopped tile must read 0 */
        const bool budget = passes || (budgetActive_ && select);
        if (converge_) meterShown(shown, /*sync=*/!varGuided_ && !denoise_ && !select && !budget, noiseMapReadback_ || adapt);
        if (select && adaptHist) { /* ... gated by the shortest kept length of each tile's surface pixels */
            b.tileLen.need(noiseTileCount(), "tile history lengths");
            rt_.tileLenMin(len, b.feat.p, b.tileLen.p, width_, height_, true, /*sync=*/false);
            rt_adaptive_params prm = adaptiveParams_; /* (a cap under min_frames must not keep every tile live for ever) */
            const float cap = temporalParams_.max_history;
            if (cap < (float)prm.min_frames) prm.min_frames = (uint32_t)cap; /* (cap >= 1: rt_reproject's check) */
            rt_.tileStopSelectFrames(b.noiseTiles.p, b.tileLen.p, reinterpret_cast<uint32_t *>(b.stop.p), (uint32_t)n,
                                     reinterpret_cast<rt_adaptive_stats *>(b.adaptStats.p), width_, height_, prm, true,
                                     /*sync=*/!varGuided_ && !denoise_ && !budget);
        } else if (select) /* the plane the next render is masked by, from this display's tile map */
            rt_.tileStopSelect(b.noiseTiles.p, reinterpret_cast<uint32_t *>(b.stop.p), (uint32_t)n,
                               reinterpret_cast<rt_adaptive_stats *>(b.adaptStats.p), width_, height_, adaptiveParams_, true,
                               /*sync=*/!varGuided_ && !denoise_ && !budget);
        if (budget) /* the passes of the next display, from the same map and the plane just updated */
            rt_.tileBudget(b.noiseTiles.p, reinterpret_cast<const uint32_t *>(b.stop.p), reinterpret_cast<uint32_t *>(b.passes.p),
                           reinterpret_cast<rt_budget_stats *>(b.budgetStats.p), width_, height_, budgetParams_, true,
                           /*sync=*/!varGuided_ && !denoise_);
        if (varGuided_) { /* in place of setDenoise's filter, whether that is on or not */
            rt_.denoiseVar(shown, b.var.p, b.feat.p, b.den.p, nullptr, width_, height_, varParams_, true);
            shown = b.den.p;
        } else if (denoise_) {
            rt_.denoise(shown, b.feat.p, b.den.p, width_, height_, denoiseParams_, true);
            shown = b.den.p;
        }
        if (toneMap_) toneMapShown(shown);
        if (!toneMap_ || floatReadback_) { /* (else the 8-bit frame alone: pixels() keeps its last contents) */
            if (shown == b.dev.p && !passes) /* nothing is switched on: the non-sharing readback into the PBO */
                rt_.read(pbo_.data(), pbo_.size()); /* (the tracer's last target; in the pass loop that is the scratch frame) */
            else if (hipMemcpy(pbo_.data(), shown, 4 * px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                throw std::runtime_error("ProgressiveViewHIP: displayed frame readback failed");
        }
        if (toneMap_) {
            pbo8_.resize(px);
            if (hipMemcpy(pbo8_.data(), b.tone8.p, px * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
                throw std::runtime_error("ProgressiveViewHIP: 8-bit frame readback failed");
        }
        if (converge_) { /* the meter's sixteen bytes, and the decision they allow */
            bool ok = hipMemcpy(&noiseStats_, b.noiseStats.p, sizeof noiseStats_, hipMemcpyDeviceToHost) == hipSuccess;
            if (ok && noiseMapReadback_) {
                noiseMap_.resize(2 * noiseTileCount());
                ok = hipMemcpy(noiseMap_.data(), b.noiseTiles.p, noiseMap_.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
            }
            if (!ok) throw std::runtime_error("ProgressiveViewHIP: noise stats readback failed");
            converged_ = frames_ >= convergeMinFrames_ && noiseStats_.counted > 0 && noiseStats_.level <= convergeParams_.threshold;
        }
        if (adapt) { /* the stop rule's sixteen bytes, and the other way to be done: no tile is live */
            const uint32_t tiles = (uint32_t)noiseTileCount();
            adaptiveStats_ = rt_adaptive_stats{tiles, tiles, 0u, (uint32_t)n}; /* before the first select the plane is zero */
            bool ok = !select || hipMemcpy(&adaptiveStats_, b.adaptStats.p, sizeof adaptiveStats_, hipMemcpyDeviceToHost) == hipSuccess;
            if (ok && stopMapReadback_) {
                stopMap_.resize(tiles);
                ok = hipMemcpy(stopMap_.data(), b.stop.p, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
            }
            if (!ok) throw std::runtime_error("ProgressiveViewHIP: stop rule readback failed");
            converged_ = converged_ || adaptiveStats_.active == 0u;
        }
        if (budget) { /* the budget's words, with the frame's other small readbacks */
            bool ok = hipMemcpy(&budgetStats_, b.budgetStats.p, sizeof budgetStats_, hipMemcpyDeviceToHost) == hipSuccess;
            haveBudget_ = ok;
            if (!ok) throw std::runtime_error("ProgressiveViewHIP: budget stats readback failed");
        }
        if (budgetActive_ && countReadback_) {
            sampleCounts_.resize(noiseTileCount());
            if (hipMemcpy(sampleCounts_.data(), b.count.p, sampleCounts_.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
                throw std::runtime_error("ProgressiveViewHIP: count plane readback failed");
        }
        if (temporal_ && histLenReadback_) {
            histLen_.resize(px);
            if (hipMemcpy(histLen_.data(), b.colour.kept.len(), px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                throw std::runtime_error("ProgressiveViewHIP: history length readback failed");
        }
        if (sphereCarry_ && kernel_ != RT_KERNEL_TRIS) { /* the spheres this frame was displayed with */
            shownSpheres_ = rt_.spheres();
            shownValid_ = true;
        }
        rendered_ = true;
    }

    RayTracerHIP &rt_;
    unsigned width_, height_;
    int kernel_;
    std::unique_ptr<Buffers> buf_; /* never null: a reshape frees the lot by starting a new one */
    bool denoise_ = false, featDirty_ = true;
    /* setTemporal: the camera of the kept frame; whether there is one; whether this display carries it */
    rt_camera histCam_{};
    bool temporal_ = false, haveHist_ = false, carry_ = false;
    bool motionCarry_ = false, posePending_ = false;
    float motionMaxHistory_ = 8.0f;
    /* setSphereCarry: the sphere list of the last traced display, whether it is one, whether a change is to be carried */
    bool sphereCarry_ = false, shownValid_ = false, spheresPending_ = false;
    float sphereMaxHistory_ = 8.0f;
    std::vector<rt_sphere> shownSpheres_;
    bool trust_ = false;
    rt_trust_params trustParams_ = RayTracerHIP::trustDefaults();
    rt_reproject_params temporalParams_ = RayTracerHIP::reprojectDefaults();
    rt_denoise_params denoiseParams_ = RayTracerHIP::denoiseDefaults();
    bool varGuided_ = false, momValid_ = false;
    rt_denoise_var_params varParams_ = RayTracerHIP::denoiseVarDefaults();
    /* setConverge: on; whether the last traced display converged; the frames in the view's moments */
    bool converge_ = false, converged_ = false, noiseMapReadback_ = false;
    unsigned convergeMinFrames_ = 8, frames_ = 0;
    rt_noise_params convergeParams_ = RayTracerHIP::noiseDefaults();
    rt_noise_stats noiseStats_{};
    std::vector<float> noiseMap_;
    /* setAdaptive: on; the plane is to be zeroed before the next render; the plane the tracer borrows (null: none) */
    bool adaptive_ = false, stopReset_ = true, stopMapReadback_ = false;
    bool adaptHistory_ = false; /* setAdaptiveHistory */
    bool histLenReadback_ = false;
    std::vector<float> histLen_;
    const float *plane_ = nullptr;
    /* setSampleBudget: on; in effect (from a display with zeroed planes on); a budget has run since the planes were zeroed */
    bool budget_ = false, budgetActive_ = false, haveBudget_ = false, countReadback_ = false;
    rt_budget_params budgetParams_ = RayTracerHIP::budgetDefaults();
    rt_budget_stats budgetStats_{};
    std::vector<uint32_t> sampleCounts_;
    rt_adaptive_params adaptiveParams_ = RayTracerHIP::adaptiveDefaults();
    rt_adaptive_stats adaptiveStats_{};
    std::vector<uint32_t> stopMap_;
    bool toneMap_ = false, autoExposure_ = true, exposureReset_ = true, floatReadback_ = true;
    rt_tonemap_params toneParams_ = RayTracerHIP::toneMapDefaults();
    rt_meter_params meterParams_ = RayTracerHIP::meterDefaults();
    std::vector<uint32_t> pbo8_;
    std::vector<float> pbo_, raw_;
    bool realloc_ = true, rendered_ = false;
    unsigned progression_ = 0, maxProgression_ = 10000;
    float azimuth_ = 105.0f, elevation_ = 40.0f, distance_ = 5.0f;
};

#endif /* PROGRESSIVE_VIEW_HIP_HPP */
