// tests/cpp/gl_pbo_rgba8.cpp — TEST PROGRAM: the RGBA8 form of include/GlPboTargetHIP.hpp (the
// tone-mapped frame in a PBO of 4 bytes per pixel), compiled and linked against
// libGL, the HIP runtime and librtmi.  There is no GL context here or on the GPU box, so, like
// gl_pbo_target.cpp, it only checks that the adapter builds; a desktop session with a current GL
// context runs both PBO paths (run with `window`: not automated here).
#define GL_GLEXT_PROTOTYPES 1
#include "GlPboTargetHIP.hpp"

#include <cstdio>
#include <cstring>

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "window")) { /* needs a current GL context and a PBO */
        GLuint pbo = 0;
        glGenBuffers(1, &pbo);
        glBindBuffer(GL_PIXEL_UNPACK_BUFFER, pbo);
        glBufferData(GL_PIXEL_UNPACK_BUFFER, 64 * 64 * 4, nullptr, GL_DYNAMIC_DRAW);
        glBindBuffer(GL_PIXEL_UNPACK_BUFFER, 0);
        RayTracerHIP rt;
        rt_meter_params meter = RayTracerHIP::meterDefaults();
        meter.rate = 0.25f;
        for (int sharing = 1; sharing >= 0; --sharing) {
            GlPboTargetHIP target(pbo, 64, 64, sharing != 0, GlPboTargetHIP::RGBA8);
            target.setToneMap(RayTracerHIP::toneMapDefaults(), true, meter);
            for (unsigned p = 0; p < 3; ++p) target.rayTrace(rt, p);
            std::printf("sharing=%d bytes=%zu ok\n", (int)target.sharing(), target.pboBytes());
        }
        return 0;
    }
    std::printf("built: float target %d, RGBA8 target %d\n", (int)GlPboTargetHIP::RGBA32F, (int)GlPboTargetHIP::RGBA8);
    return 0;
}
