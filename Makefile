# Build of the MI355X path-tracing hot path.
#   librtpt.so   gfx950 HIP kernel + C-ABI (include/rtpt.h)     -> gpuraytracer_amd/
#   rtrace       C++ CLI host (mirrors RTrace/main.swift)       -> gpuraytracer_amd/
#   oracle       CPU oracle for tests / cpu_baseline            -> oracle/liboracle.so
# Every TU is compiled with -ffp-contract=off: the arithmetic contract of
# DESIGN.md §3 (explicit fmaf only) that makes GPU == oracle bit-exact.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := gpuraytracer_amd
SRC := $(PKG)/csrc
BLD ?= build
COMMON := -std=c++17 -O3 -fPIC -ffp-contract=off -Wall -Wno-unused-function -Iinclude
HOSTCXX ?= /opt/rocm/llvm/bin/clang++
HIPFLAGS := $(COMMON) --offload-arch=$(ARCH) -fno-slp-vectorize $(EXTRA)
HOSTFLAGS := $(COMMON) -D__HIP_PLATFORM_AMD__ -isystem /opt/rocm/include $(EXTRA)

# The library's objects, named once: the device ones (.hip) and the host ones
# (.cpp), which the sanitizer build below compiles a second time.
DEV_OBJS := rt_kernel.o rt_rays.o rt_aov.o rt_denoise.o rt_reproject.o rt_adaptive.o rt_mis.o rt_lbvh.o rt_gsah.o rt_refit.o rt_mathcheck.o
HOST_OBJS := rt_api.o rt_api_host.o rt_scene.o rt_camera.o rt_reproject_host.o rt_image.o
OBJS := $(addprefix $(BLD)/,$(DEV_OBJS) $(HOST_OBJS))
HDRS := include/rtpt.h include/rt_types.h $(SRC)/rt_math.h $(SRC)/rt_kernel.hpp $(SRC)/rt_scene.hpp $(SRC)/rt_halton.hpp $(SRC)/rt_beam.hpp $(SRC)/rt_shaft.hpp $(SRC)/rt_cluorder.hpp $(SRC)/rt_raydomain.h $(SRC)/rt_pixel.hpp $(SRC)/rt_plan.hpp $(SRC)/rt_wavemask.hpp

LIB ?= $(PKG)/librtpt.so
# Hash of every source the library is built from (gpuraytracer_amd/srchash.py),
# compiled into rt_api.o as rt_build_sha(): the loader refuses a stale binary.
ALLSRC := $(wildcard $(SRC)/*.hip $(SRC)/*.hpp $(SRC)/*.h $(SRC)/*.cpp include/*.h)
SRC_SHA := $(shell python3 $(PKG)/srchash.py)

all: $(LIB) $(PKG)/rtrace oracle

lib: $(LIB)

$(BLD):
	mkdir -p $(BLD)

$(BLD)/%.o: $(SRC)/%.hip $(HDRS) $(SRC)/rt_trace.hpp | $(BLD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the device-vs-host check of the shared scalar functions
$(BLD)/rt_mathcheck.o $(BLD)/rt_image.o $(BLD)/rt_api_host.o: $(SRC)/rt_half.h $(SRC)/rt_mathcheck.hpp
$(BLD)/rt_api_host.o $(BLD)/rt_reproject_host.o: $(SRC)/rt_api_internal.hpp $(SRC)/rt_reproject.hpp
$(BLD)/rt_reproject.o: $(SRC)/rt_reproject.hpp
$(BLD)/rt_kernel.o: $(SRC)/rt_free.hpp $(SRC)/rt_counts.hpp $(SRC)/rt_paths.hpp

$(BLD)/rt_api.o: $(SRC)/rt_api.cpp $(ALLSRC) | $(BLD)
	$(HOSTCXX) $(HOSTFLAGS) -DRT_SRC_SHA='"$(SRC_SHA)"' -c $< -o $@

$(BLD)/%.o: $(SRC)/%.cpp $(HDRS) | $(BLD)
	$(HOSTCXX) $(HOSTFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) -shared --offload-arch=$(ARCH) -o $@ $(OBJS) -L/opt/rocm/lib -lrccl -Wl,--no-undefined

$(PKG)/rtrace: $(SRC)/rtrace_main.cpp $(PKG)/librtpt.so $(HDRS)
	$(HOSTCXX) $(HOSTFLAGS) -o $@ $< -L$(PKG) -lrtpt -Wl,-rpath,'$$ORIGIN'

oracle:
	$(MAKE) -C oracle

# ---- sanitizer build of the CPU code (ASan/UBSan) -------------------
# build_asan/liboracle.so  the oracle, -fsanitize=address,undefined
# build_asan/librtpt.so    the host C++ of the library (scene compile, host BVH
#                          builds on host threads, tile layout/placement, image
#                          epilogue, C-ABI argument handling) sanitized, linked
#                          with the device objects of build/
# `make asan-test` runs the CPU tests of that code (tests/run_sanitized.py)
# under it; UBSan findings abort (-fno-sanitize-recover).
ASAN := build_asan
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -shared-libasan
ASAN_RT := $(shell $(HOSTCXX) -print-file-name=libclang_rt.asan-x86_64.so)
ASAN_HOST := $(addprefix $(ASAN)/,$(HOST_OBJS))

$(ASAN):
	mkdir -p $(ASAN)

$(ASAN)/rt_api.o: $(SRC)/rt_api.cpp $(ALLSRC) | $(ASAN)
	$(HOSTCXX) $(HOSTFLAGS) $(SAN) -DRT_SRC_SHA='"$(SRC_SHA)"' -c $< -o $@

$(ASAN)/%.o: $(SRC)/%.cpp $(HDRS) | $(ASAN)
	$(HOSTCXX) $(HOSTFLAGS) $(SAN) -c $< -o $@

$(ASAN)/rt_image.o $(ASAN)/rt_api_host.o: $(SRC)/rt_half.h
$(ASAN)/rt_api_host.o: $(SRC)/rt_api_internal.hpp $(SRC)/rt_mathcheck.hpp
$(ASAN)/rt_api_host.o $(ASAN)/rt_reproject_host.o: $(SRC)/rt_reproject.hpp
$(ASAN)/rt_reproject_host.o: $(SRC)/rt_api_internal.hpp

$(ASAN)/librtpt.so: $(ASAN_HOST) $(addprefix $(BLD)/,$(DEV_OBJS))
	$(HOSTCXX) -shared $(SAN) -o $@ $^ -L/opt/rocm/lib -lamdhip64 -lrccl -Wl,-rpath,/opt/rocm/lib

$(ASAN)/liboracle.so: oracle/pt_oracle.c oracle/pt_oracle.h include/rt_types.h | $(ASAN)
	$(HOSTCXX:clang++=clang) -x c -std=c11 -O1 -mfma -ffp-contract=off -fno-fast-math -fPIC -Wall -pthread \
	    $(SAN) -shared -o $@ oracle/pt_oracle.c -lm

asan: $(ASAN)/librtpt.so $(ASAN)/liboracle.so

asan-test: asan
	RTPT_SAN_DIR=$(abspath $(ASAN)) RTPT_SAN_RT=$(ASAN_RT) python3 tests/run_sanitized.py

# Stand-alone sanitizer run of rt_reproject_host (tools/reproject_host_check.cpp):
# a program with its own main, linked with the sanitized host objects it needs
# and nothing of the device side, over adversarial buffers and tiny frames.
$(ASAN)/reproject_host_check: tools/reproject_host_check.cpp $(ASAN)/rt_reproject_host.o $(ASAN)/rt_camera.o
	$(HOSTCXX) $(HOSTFLAGS) $(SAN:-shared-libasan=) -o $@ $^

reproject-check: $(ASAN)/reproject_host_check
	$(ASAN)/reproject_host_check

clean:
	rm -rf $(BLD) $(ASAN) $(PKG)/librtpt.so $(PKG)/rtrace
	$(MAKE) -C oracle clean

.PHONY: all lib oracle clean asan asan-test reproject-check
