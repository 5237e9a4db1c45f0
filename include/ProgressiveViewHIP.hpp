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
 */
#ifndef PROGRESSIVE_VIEW_HIP_HPP
#define PROGRESSIVE_VIEW_HIP_HPP

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "RayTracerHIP.hpp"

class ProgressiveViewHIP {
public:
    enum Key { KEY_LEFT, KEY_RIGHT, KEY_UP, KEY_DOWN };

    ProgressiveViewHIP(RayTracerHIP &rt, unsigned width, unsigned height, int kernel = RT_KERNEL_SPHERES)
        : rt_(rt), width_(width), height_(height), kernel_(kernel)
    {
    }
    ~ProgressiveViewHIP() { release(); }
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
            again = maxProgression_ > 0;
        } else if (progression_ < maxProgression_) {
            ++progression_;
            trace();
            again = true;
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
        const bool post = progression_ >= maxProgression_;
        progression_ = 0;
        carry_ = true;
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
        if (carryMotion && !(posePending_ && poseVerts_ == n_verts)) {
            if (poseVerts_ != n_verts) {
                if (posePrev_) (void)hipFree(posePrev_);
                posePrev_ = nullptr;
                poseVerts_ = n_verts;
            }
            alloc(posePrev_, (size_t)n_verts * 3 * sizeof(float), "pose snapshot");
            rt_.meshPose(posePrev_, n_verts, true);
            posePending_ = true;
        }
        rt_.updateMesh(verts_xyz, n_verts, flags);
        featDirty_ = true;
        if (!carryMotion) {
            haveHist_ = false;
            momValid_ = false;
            posePending_ = false;
        }
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
    /* The spheres have changed (the caller's addSphere / clearSpheres).  Without setHistoryTrust the
       history and the moments show the old lighting and are dropped; with it they are kept and judged.
       Progression back to 0; returns restart()'s answer. */
    bool sceneChanged()
    {
        featDirty_ = true;
        if (!trust_) {
            haveHist_ = false;
            momValid_ = false;
            posePending_ = false;
        }
        const bool post = restart();
        if (!trust_) carry_ = false;
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
            haveHist_ = false;
            posePending_ = false;
        }
        temporal_ = on;
        temporalParams_ = params;
    }
    bool temporal() const { return temporal_; }
    void setVarianceGuided(bool on, const rt_denoise_var_params &params = RayTracerHIP::denoiseVarDefaults())
    {
        if (on && !varGuided_) {
            featDirty_ = true;
            haveHist_ = false;
            momValid_ = false;
            posePending_ = false;
        }
        varGuided_ = on;
        varParams_ = params;
    }
    bool varianceGuided() const { return varGuided_; }

    const std::vector<float> &pixels() const { return pbo_; }
    /* The accumulation buffer as rendered (what pixels() holds with the denoiser off), read back now. */
    const std::vector<float> &rawPixels()
    {
        if (!denoise_ && !temporal_ && !varGuided_) return pbo_;
        raw_.assign(pbo_.size(), 0.0f);
        if (dev_ && hipMemcpy(raw_.data(), dev_, raw_.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
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
    void allocate()
    {
        release();
        if (hipMalloc(&dev_, (size_t)width_ * height_ * 4 * sizeof(float)) != hipSuccess)
            throw std::runtime_error("ProgressiveViewHIP: framebuffer allocation failed");
        pbo_.assign((size_t)width_ * height_ * 4, 0.0f);
        featDirty_ = true;
        haveHist_ = false;
        momValid_ = false;
        posePending_ = false;
    }
    void release()
    {
        if (dev_) (void)hipFree(dev_);
        if (den_) (void)hipFree(den_);
        if (feat_) (void)hipFree(feat_);
        if (featPrev_) (void)hipFree(featPrev_);
        if (hist_) (void)hipFree(hist_);
        if (carried_) (void)hipFree(carried_);
        for (float *b : {accPrev_, mom_, momHist_, momCarried_, var_, len_, featWarp_, posePrev_, trustLen_})
            if (b) (void)hipFree(b);
        dev_ = den_ = feat_ = featPrev_ = hist_ = carried_ = nullptr;
        accPrev_ = mom_ = momHist_ = momCarried_ = var_ = len_ = featWarp_ = posePrev_ = trustLen_ = nullptr;
        poseVerts_ = 0;
    }
    void alloc(float *&buf, size_t bytes, const char *what)
    {
        if (!buf && hipMalloc(&buf, bytes) != hipSuccess)
            throw std::runtime_error(std::string("ProgressiveViewHIP: ") + what + " allocation failed");
    }
    /* the merged frame of this display into hist_ (colour, then its plane of history lengths); with
       setVarianceGuided the view's moments mom_ go the same way into momHist_ */
    void mergeTemporal()
    {
        const size_t px = (size_t)width_ * height_, frame = px * 4 * sizeof(float);
        /* hist_ / carried_: a colour frame followed by its plane of history lengths */
        alloc(feat_, 2 * frame, "feature buffer");
        alloc(featPrev_, 2 * frame, "feature buffer");
        alloc(hist_, frame + px * sizeof(float), "history buffer");
        alloc(carried_, frame + px * sizeof(float), "history buffer");
        if (varGuided_) {
            alloc(momHist_, frame + px * sizeof(float), "moments history buffer");
            alloc(momCarried_, frame + px * sizeof(float), "moments history buffer");
        }
        const rt_camera cam = rt_.getCamera(width_);
        const float *histFeat = feat_; /* the features of the view the kept frame was displayed in */
        if (featDirty_) {
            std::swap(feat_, featPrev_);
            histFeat = featPrev_;
            rt_.renderFeatures(feat_, width_, height_, kernel_, true);
            featDirty_ = false;
            carry_ = true;
        }
        const bool judged = trust_ && haveHist_; /* a history exists: it is judged at every display */
        if (!haveHist_) { /* after a (re)allocation: no history anywhere */
            if (hipMemset(carried_, 0, frame + px * sizeof(float)) != hipSuccess ||
                (varGuided_ && hipMemset(momCarried_, 0, frame + px * sizeof(float)) != hipSuccess) ||
                hipDeviceSynchronize() != hipSuccess)
                throw std::runtime_error("ProgressiveViewHIP: history reset failed");
        } else if (carry_) { /* a new accumulation begins: carry the kept frame into it */
            const float *curFeat = feat_;
            rt_reproject_params prm = temporalParams_;
            if (posePending_) { /* the mesh has moved since: the taps are sought where the material was */
                alloc(featWarp_, 2 * frame, "feature buffer");
                rt_.warpFeatures(feat_, posePrev_, poseVerts_, featWarp_, width_, height_, true);
                curFeat = featWarp_;
                prm.max_history = std::fmin(temporalParams_.max_history, motionMaxHistory_);
            }
            rt_.reproject(hist_, hist_ + 4 * px, histFeat, histCam_, curFeat, carried_, carried_ + 4 * px, width_, height_, prm,
                          true);
            if (varGuided_) /* the same lengths, features and cameras: the colour's taps and weights */
                rt_.reproject(momHist_, hist_ + 4 * px, histFeat, histCam_, curFeat, momCarried_, momCarried_ + 4 * px, width_,
                              height_, prm, true);
        }
        posePending_ = false;
        carry_ = false;
        const float n = (float)(progression_ > 1 ? progression_ : 1);
        /* the lengths the merges blend by: the carried ones, or with setHistoryTrust what this display's
           accumulation buffer leaves of them (one plane for colour and moments: they keep one length) */
        const float *colLen = carried_ + 4 * px, *momLen = varGuided_ ? momCarried_ + 4 * px : nullptr;
        if (judged) {
            alloc(trustLen_, px * sizeof(float), "trusted history length buffer");
            rt_.historyTrust(carried_, carried_ + 4 * px, dev_, n, feat_, trustLen_, width_, height_, trustParams_, true);
            colLen = momLen = trustLen_;
        }
        rt_.temporalMerge(carried_, colLen, dev_, n, temporalParams_.max_history, hist_, hist_ + 4 * px, width_, height_, true);
        if (varGuided_)
            rt_.temporalMerge(momCarried_, momLen, mom_, n, temporalParams_.max_history, momHist_, momHist_ + 4 * px, width_,
                              height_, true);
        histCam_ = cam;
        haveHist_ = true;
    }
    void traceTemporal()
    {
        const size_t frame = (size_t)width_ * height_ * 4 * sizeof(float);
        if (denoise_) alloc(den_, frame, "denoised framebuffer");
        mergeTemporal();
        const float *shown = hist_;
        if (denoise_) {
            rt_.denoise(hist_, feat_, den_, width_, height_, denoiseParams_, true);
            shown = den_;
        }
        if (hipMemcpy(pbo_.data(), shown, frame, hipMemcpyDeviceToHost) != hipSuccess)
            throw std::runtime_error("ProgressiveViewHIP: displayed frame readback failed");
    }
    /* before a render that refines the accumulation buffer: its copy, for the frame's own sample */
    void keepAccumulation()
    {
        const size_t frame = (size_t)width_ * height_ * 4 * sizeof(float);
        alloc(accPrev_, frame, "accumulation copy");
        if (progression_ > 1 &&
            (hipMemcpy(accPrev_, dev_, frame, hipMemcpyDeviceToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess))
            throw std::runtime_error("ProgressiveViewHIP: accumulation copy failed");
    }
    void traceVarianceGuided()
    {
        const size_t px = (size_t)width_ * height_, frame = px * 4 * sizeof(float);
        alloc(mom_, frame, "moments buffer");
        alloc(var_, px * sizeof(float), "variance buffer");
        alloc(den_, frame, "denoised framebuffer");
        /* (without valid moments, after it was switched on in mid-accumulation: start from this frame) */
        const float n = (float)(progression_ > 1 ? progression_ : 1);
        rt_.momentsAccumulate(accPrev_, dev_, momValid_ ? n : 1.0f, mom_, mom_, width_, height_, true);
        momValid_ = true;
        const float *shown = dev_, *moments = mom_, *len = nullptr;
        if (temporal_) {
            mergeTemporal();
            shown = hist_;
            moments = momHist_;
            len = hist_ + 4 * px;
        } else {
            alloc(feat_, 2 * frame, "feature buffer");
            alloc(len_, px * sizeof(float), "history length buffer");
            if (featDirty_) {
                rt_.renderFeatures(feat_, width_, height_, kernel_, true);
                featDirty_ = false;
            }
            const std::vector<float> lens(px, n); /* one view, n frames everywhere */
            if (hipMemcpy(len_, lens.data(), px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
                throw std::runtime_error("ProgressiveViewHIP: history length upload failed");
            len = len_;
        }
        rt_.variance(shown, moments, len, feat_, var_, width_, height_, varParams_, true);
        rt_.denoiseVar(shown, var_, feat_, den_, nullptr, width_, height_, varParams_, true);
        if (hipMemcpy(pbo_.data(), den_, frame, hipMemcpyDeviceToHost) != hipSuccess)
            throw std::runtime_error("ProgressiveViewHIP: displayed frame readback failed");
    }
    void trace()
    {
        if (varGuided_) keepAccumulation();
        rt_.rayTrace(dev_, width_, height_, progression_, kernel_, true);
        if (varGuided_) {
            traceVarianceGuided();
        } else if (temporal_) {
            traceTemporal();
        } else if (denoise_) {
            const size_t frame = (size_t)width_ * height_ * 4 * sizeof(float);
            if (!den_ && hipMalloc(&den_, frame) != hipSuccess)
                throw std::runtime_error("ProgressiveViewHIP: denoised framebuffer allocation failed");
            if (!feat_ && hipMalloc(&feat_, 2 * frame) != hipSuccess)
                throw std::runtime_error("ProgressiveViewHIP: feature buffer allocation failed");
            if (featDirty_) {
                rt_.renderFeatures(feat_, width_, height_, kernel_, true);
                featDirty_ = false;
            }
            rt_.denoise(dev_, feat_, den_, width_, height_, denoiseParams_, true);
            if (hipMemcpy(pbo_.data(), den_, frame, hipMemcpyDeviceToHost) != hipSuccess)
                throw std::runtime_error("ProgressiveViewHIP: denoised frame readback failed");
        } else {
            rt_.read(pbo_.data(), pbo_.size()); /* the non-sharing readback into the PBO */
        }
        rendered_ = true;
    }

    RayTracerHIP &rt_;
    unsigned width_, height_;
    int kernel_;
    float *dev_ = nullptr;  /* the accumulation buffer the tracer renders into */
    float *den_ = nullptr;  /* setDenoise: the filtered frame */
    float *feat_ = nullptr; /* setDenoise: the view's first-hit features */
    bool denoise_ = false, featDirty_ = true;
    /* setTemporal: the last displayed frame (merged colour + history length), its features and
       camera; the history carried into the current view (colour + length) */
    float *hist_ = nullptr, *featPrev_ = nullptr, *carried_ = nullptr;
    rt_camera histCam_{};
    bool temporal_ = false, haveHist_ = false, carry_ = false;
    /* setMotionCarry: the pose the kept frame was displayed in (a device copy taken at the first
       updateMesh after a display), and the current features warped into it */
    float *posePrev_ = nullptr, *featWarp_ = nullptr;
    uint32_t poseVerts_ = 0;
    bool motionCarry_ = false, posePending_ = false;
    float motionMaxHistory_ = 8.0f;
    /* setHistoryTrust: the plane of history lengths the carried history still deserves at this display */
    float *trustLen_ = nullptr;
    bool trust_ = false;
    rt_trust_params trustParams_ = RayTracerHIP::trustDefaults();
    rt_reproject_params temporalParams_ = RayTracerHIP::reprojectDefaults();
    rt_denoise_params denoiseParams_ = RayTracerHIP::denoiseDefaults();
    /* setVarianceGuided: the accumulation buffer before the frame, the view's moments, with
       setTemporal their merged and carried histories (moments + length plane, as hist_ / carried_),
       the variance plane and (without setTemporal) the plane of history lengths */
    float *accPrev_ = nullptr, *mom_ = nullptr, *momHist_ = nullptr, *momCarried_ = nullptr, *var_ = nullptr,
          *len_ = nullptr;
    bool varGuided_ = false, momValid_ = false;
    rt_denoise_var_params varParams_ = RayTracerHIP::denoiseVarDefaults();
    std::vector<float> pbo_, raw_;
    bool realloc_ = true, rendered_ = false;
    unsigned progression_ = 0, maxProgression_ = 10000;
    float azimuth_ = 105.0f, elevation_ = 40.0f, distance_ = 5.0f;
};

#endif /* PROGRESSIVE_VIEW_HIP_HPP */
