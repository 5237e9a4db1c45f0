# tests/cpp/light_cone.mk — TEST PROGRAM: host_cone_dump, host_tree_dump with the lights' radii (the
# shadow tree with the cone split, tests/test_light_cone_host.py).  Plain host C++ with the flags of
# host_tree_dump in the Makefile beside it, rt_bvh.cpp and the program's main only.
#   make -C tests/cpp -f light_cone.mk
LIB   := ../../pathtracer.cl_amd
CLANG := /opt/rocm/lib/llvm/bin/clang

host_cone_dump: host_cone_dump.cpp $(LIB)/csrc/rt_bvh.cpp $(LIB)/csrc/rt_internal.h $(LIB)/csrc/rt_quant.h
	$(CLANG)++ -O3 -std=c++17 -ffp-contract=off -fno-fast-math -Wall -I../../include -I$(LIB)/csrc -o $@ \
	    host_cone_dump.cpp $(LIB)/csrc/rt_bvh.cpp

clean:
	rm -f host_cone_dump

.PHONY: clean
