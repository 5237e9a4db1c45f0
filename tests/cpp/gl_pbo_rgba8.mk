# tests/cpp/gl_pbo_rgba8.mk — TEST PROGRAM: gl_pbo_rgba8, the RGBA8 form of include/GlPboTargetHIP.hpp
# compiled and linked against libGL, the HIP runtime and librtmi with gl_pbo_target's flags in the
# Makefile beside it (tests/test_tonemap_host.py).  No GL context anywhere: compile and link only.
#   make -C tests/cpp -f gl_pbo_rgba8.mk
HIPCC ?= /opt/rocm/bin/hipcc
LIB   := ../../pathtracer.cl_amd

gl_pbo_rgba8: gl_pbo_rgba8.cpp ../../include/GlPboTargetHIP.hpp ../../include/RayTracerHIP.hpp $(LIB)/librtmi.so
	$(HIPCC) -O2 -std=c++17 --offload-arch=gfx950 -DRT_HIP_NO_REFERENCE_TYPES -I../../include -o $@ gl_pbo_rgba8.cpp \
	    -L$(LIB) -lrtmi -lGL -Wl,-rpath,'$$ORIGIN/$(LIB)'

clean:
	rm -f gl_pbo_rgba8

.PHONY: clean
