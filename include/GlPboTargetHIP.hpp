/*
 * GlPboTargetHIP.hpp — the display side of GlutCLWindow::rayTrace (clrt/GlutCLWindow.cpp:190-227)
 * for RayTracerHIP: renders a frame into an OpenGL pixel-unpack buffer (PBO).
 *
 * GlutCLWindow has two paths, chosen by RayTracerCL::supportsGLSharing():
 *   sharing     clEnqueueAcquireGLObjects on the PBO, rayTrace(&clPBO, ...) writes the frame
 *               straight into it, clEnqueueReleaseGLObjects hands it back to GL (:196-212);
 *   no sharing  rayTrace into a CL buffer, then glMapBuffer(GL_PIXEL_UNPACK_BUFFER, WRITE_ONLY)
 *               and a blocking enqueueReadBuffer into the mapped PBO (:213-226).
 * Here the same two paths:
 *   sharing     hipGraphicsGLRegisterBuffer once per PBO, then per frame
 *               hipGraphicsMapResources → hipGraphicsResourceGetMappedPointer → rt_render with
 *               RT_OUT_DEVICE into the PBO's memory → hipGraphicsUnmapResources;
 *   no sharing  (registration refused: no GL context on the GPU's device, a remote display)
 *               rt_render into a device framebuffer this object owns, then glMapBuffer and
 *               rt_read (the blocking readback) into the mapped PBO.
 * The PBO is registered without WriteDiscard: a progressive frame (progression p > 0) mixes
 * with the frame already in it (GlutCLWindow.cpp:144-158), exactly as the CL kernel read the
 * shared buffer.  In the fallback the device framebuffer carries the accumulated frame, as
 * the reference's clPBOBuff did.
 *
 * Needs a current GL context with GL_PIXEL_UNPACK_BUFFER (GL 2.1 / ARB_pixel_buffer_object)
 * and GL_GLEXT_PROTOTYPES (or a loader) for glBindBuffer / glMapBuffer, and linking with
 * -lGL.  Only the window's rayTrace() changes:
 *
 *     GlPboTargetHIP target(pbo, width, height);        // allocatePBO()
 *     target.rayTrace(rayTracer, progression);          // rayTrace()
 *     target.resize(pbo, width, height);                // reshape: a new PBO
 *
 * The RGBA8 form (format = RGBA8; nothing in the reference corresponds to it): the PBO
 * holds 4 bytes per pixel, the tone-mapped frame (rt_tonemap's words: GL_RGBA / GL_UNSIGNED_BYTE in
 * memory), so the caller draws it with glDrawPixels(w, h, GL_RGBA, GL_UNSIGNED_BYTE, 0) in place of
 * GL_FLOAT.  The accumulated float frame then always lives in a device framebuffer this object owns;
 * every rayTrace meters it (setToneMap: auto-exposure, the exposure float kept on the device) and
 * tone-maps it straight into the shared PBO, or into a device buffer read back into the mapped PBO —
 * a quarter of the float form's bytes.  The float form stays the default.
 */
#ifndef GL_PBO_TARGET_HIP_HPP
#define GL_PBO_TARGET_HIP_HPP

#include <GL/gl.h>
#include <GL/glext.h>
#include <hip/hip_runtime_api.h> /* before the interop header, which uses its types */
#include <hip/hip_gl_interop.h>

#include <cstddef>
#include <stdexcept>
#include <string>

#include "RayTracerHIP.hpp"

class GlPboTargetHIP {
public:
    enum Format { RGBA32F, RGBA8 }; /* of the PBO: 16 or 4 bytes per pixel */

    /* try_sharing = false forces the readback path (RayTracerCL's supportsGLSharing() false) */
    GlPboTargetHIP(GLuint pbo, unsigned width, unsigned height, bool try_sharing = true, Format format = RGBA32F)
        : try_sharing_(try_sharing), format_(format)
    {
        attach(pbo, width, height);
    }
    ~GlPboTargetHIP() { detach(); }
    GlPboTargetHIP(const GlPboTargetHIP &) = delete;
    GlPboTargetHIP &operator=(const GlPboTargetHIP &) = delete;

    /* a reshaped window's new PBO (GlutCLWindow::allocatePBO after reshape) */
    void resize(GLuint pbo, unsigned width, unsigned height)
    {
        detach();
        attach(pbo, width, height);
    }

    bool sharing() const { return res_ != nullptr; }
    Format format() const { return format_; }
    size_t pboBytes() const { return (size_t)w_ * h_ * (format_ == RGBA8 ? 4 : 16); }
    /* RGBA8: the tone map's parameters; the exposure starts afresh at every attach (a reshape) */
    void setToneMap(const rt_tonemap_params &params, bool autoExposure = true,
                    const rt_meter_params &meter = RayTracerHIP::meterDefaults())
    {
        toneParams_ = params;
        autoExposure_ = autoExposure;
        meterParams_ = meter;
    }

    /* GlutCLWindow::rayTrace: one frame (kernel as RayTracerHIP::rayTrace) into the PBO */
    void rayTrace(RayTracerHIP &rt, unsigned progression, int kernel = RT_KERNEL_SPHERES)
    {
        const size_t n_floats = (size_t)w_ * h_ * 4;
        if (format_ == RGBA8) {
            rayTrace8(rt, progression, kernel);
            return;
        }
        if (res_) {
            hip(hipGraphicsMapResources(1, &res_, nullptr), "hipGraphicsMapResources");
            void *ptr = nullptr;
            size_t bytes = 0;
            hipError_t e = hipGraphicsResourceGetMappedPointer(&ptr, &bytes, res_);
            if (e == hipSuccess && bytes < n_floats * sizeof(float)) e = hipErrorInvalidValue;
            if (e != hipSuccess) {
                (void)hipGraphicsUnmapResources(1, &res_, nullptr);
                hip(e, "PBO mapped pointer (or PBO smaller than width*height*16 bytes)");
            }
            try {
                rt.rayTrace(static_cast<float *>(ptr), w_, h_, progression, kernel, /*on_device=*/true);
            } catch (...) {
                (void)hipGraphicsUnmapResources(1, &res_, nullptr);
                throw;
            }
            hip(hipGraphicsUnmapResources(1, &res_, nullptr), "hipGraphicsUnmapResources");
            return;
        }
        rt.rayTrace(frame_, w_, h_, progression, kernel, /*on_device=*/true);
        glBindBuffer(GL_PIXEL_UNPACK_BUFFER, pbo_);
        float *mapped = static_cast<float *>(glMapBuffer(GL_PIXEL_UNPACK_BUFFER, GL_WRITE_ONLY));
        if (!mapped) {
            glBindBuffer(GL_PIXEL_UNPACK_BUFFER, 0);
            throw std::runtime_error("GlPboTargetHIP: glMapBuffer(GL_PIXEL_UNPACK_BUFFER) failed");
        }
        try {
            rt.read(mapped, n_floats); /* blocking, as enqueueReadBuffer(..., CL_TRUE, ...) */
        } catch (...) {
            glUnmapBuffer(GL_PIXEL_UNPACK_BUFFER);
            glBindBuffer(GL_PIXEL_UNPACK_BUFFER, 0);
            throw;
        }
        glUnmapBuffer(GL_PIXEL_UNPACK_BUFFER);
        glBindBuffer(GL_PIXEL_UNPACK_BUFFER, 0);
    }

private:
    /* The RGBA8 form: render into the owned framebuffer, meter, tone-map into the PBO's memory (shared)
       or into the owned 8-bit buffer and from there into the mapped PBO. */
    void rayTrace8(RayTracerHIP &rt, unsigned progression, int kernel)
    {
        rt.rayTrace(frame_, w_, h_, progression, kernel, /*on_device=*/true);
        if (autoExposure_) rt.meterExposure(frame_, exposure_, nullptr, w_, h_, meterParams_, true, /*sync=*/false);
        const float *exposure = autoExposure_ ? exposure_ : nullptr;
        if (res_) {
            hip(hipGraphicsMapResources(1, &res_, nullptr), "hipGraphicsMapResources");
            void *ptr = nullptr;
            size_t bytes = 0;
            hipError_t e = hipGraphicsResourceGetMappedPointer(&ptr, &bytes, res_);
            if (e == hipSuccess && bytes < pboBytes()) e = hipErrorInvalidValue;
            if (e != hipSuccess) {
                (void)hipGraphicsUnmapResources(1, &res_, nullptr);
                hip(e, "PBO mapped pointer (or PBO smaller than width*height*4 bytes)");
            }
            try {
                rt.toneMap(frame_, exposure, static_cast<uint32_t *>(ptr), w_, h_, toneParams_, true);
            } catch (...) {
                (void)hipGraphicsUnmapResources(1, &res_, nullptr);
                throw;
            }
            hip(hipGraphicsUnmapResources(1, &res_, nullptr), "hipGraphicsUnmapResources");
            return;
        }
        rt.toneMap(frame_, exposure, frame8_, w_, h_, toneParams_, true);
        glBindBuffer(GL_PIXEL_UNPACK_BUFFER, pbo_);
        void *mapped = glMapBuffer(GL_PIXEL_UNPACK_BUFFER, GL_WRITE_ONLY);
        const hipError_t e = mapped ? hipMemcpy(mapped, frame8_, pboBytes(), hipMemcpyDeviceToHost) : hipSuccess;
        if (mapped) glUnmapBuffer(GL_PIXEL_UNPACK_BUFFER);
        glBindBuffer(GL_PIXEL_UNPACK_BUFFER, 0);
        if (!mapped) throw std::runtime_error("GlPboTargetHIP: glMapBuffer(GL_PIXEL_UNPACK_BUFFER) failed");
        hip(e, "8-bit frame readback");
    }

    static void hip(hipError_t e, const char *what)
    {
        if (e != hipSuccess)
            throw std::runtime_error(std::string("GlPboTargetHIP: ") + what + ": " + hipGetErrorString(e));
    }

    void attach(GLuint pbo, unsigned width, unsigned height)
    {
        if (!width || !height) throw std::runtime_error("GlPboTargetHIP: empty frame");
        pbo_ = pbo;
        w_ = width;
        h_ = height;
        res_ = nullptr;
        const bool shared = try_sharing_ && hipGraphicsGLRegisterBuffer(&res_, pbo, hipGraphicsRegisterFlagsNone) == hipSuccess;
        if (!shared) {
            res_ = nullptr;
            (void)hipGetLastError(); /* a refused registration is the no-sharing path, not an error */
        }
        if (shared && format_ == RGBA32F) return;
        /* (RGBA8: the float frame is this object's either way) */
        hip(hipMalloc(reinterpret_cast<void **>(&frame_), (size_t)w_ * h_ * 4 * sizeof(float)),
            "hipMalloc(framebuffer)");
        if (format_ != RGBA8) return;
        hip(hipMalloc(reinterpret_cast<void **>(&exposure_), sizeof(float)), "hipMalloc(exposure)");
        hip(hipMemset(exposure_, 0, sizeof(float)), "exposure reset"); /* 0: none yet */
        hip(hipDeviceSynchronize(), "exposure reset");
        if (!shared) hip(hipMalloc(reinterpret_cast<void **>(&frame8_), pboBytes()), "hipMalloc(8-bit framebuffer)");
    }

    void detach()
    {
        if (res_) (void)hipGraphicsUnregisterResource(res_);
        res_ = nullptr;
        if (frame_) (void)hipFree(frame_);
        frame_ = nullptr;
        if (frame8_) (void)hipFree(frame8_);
        frame8_ = nullptr;
        if (exposure_) (void)hipFree(exposure_);
        exposure_ = nullptr;
    }

    bool try_sharing_;
    GLuint pbo_ = 0;
    unsigned w_ = 0, h_ = 0;
    hipGraphicsResource_t res_ = nullptr;
    float *frame_ = nullptr; /* no-sharing path, and RGBA8: the accumulated frame on the GPU */
    Format format_ = RGBA32F;
    uint32_t *frame8_ = nullptr; /* RGBA8, no-sharing path: the tone-mapped frame on the GPU */
    float *exposure_ = nullptr;  /* RGBA8: the metered exposure (one float on the GPU) */
    rt_tonemap_params toneParams_ = RayTracerHIP::toneMapDefaults();
    bool autoExposure_ = true;
    rt_meter_params meterParams_ = RayTracerHIP::meterDefaults();
};

#endif
