# Build everything in-tree:
#   rust-path-tracer_amd/lib/librpt_hip.so   HIP kernels + C ABI (gfx950, hipcc)
#   rust-path-tracer_amd/lib/librpt_host.so  host-side dispatch mirror (g++)
#   oracle/liboracle.so, oracle/liboracle_libm.so   CPU restatement (test infrastructure)
#   oracle/libmodels_oracle.so                      the same with a material's model at lib.rs:144, and the lens too (test infrastructure; source: tests/models_oracle)
#   oracle/libvolume_oracle.so                      the models restatement with the absorption rule of rpt_set_material_volumes (test infrastructure; source: tests/volume_oracle)
#   oracle/liblights_oracle.so                      the volume restatement with the punctual lights of rpt_set_punctual_lights (test infrastructure; source: tests/lights_oracle)
#   oracle/liblens_oracle.so                        the same with the thin-lens camera at lib.rs:38-51 (test infrastructure; source: tests/lens_oracle)
# -ffp-contract=off everywhere: the parity contract forbids implicit FMA fusion.

PKG      := rust-path-tracer_amd
LIBDIR   := $(PKG)/lib
CSRC     := $(PKG)/csrc
HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++

HOST_SRCS := $(CSRC)/host/host_api.cpp $(CSRC)/host/glb_scene.cpp $(CSRC)/host/bvh_build.cpp \
             $(CSRC)/host/light_table.cpp $(CSRC)/host/bluenoise.cpp $(CSRC)/host/image_io.cpp $(CSRC)/host/textures.cpp $(CSRC)/host/obj_scene.cpp $(CSRC)/host/jpeg_decode.cpp
HIP_SRCS  := $(CSRC)/rpt_hip.hip $(CSRC)/rpt_scene.hip $(CSRC)/rpt_traverse.hip $(CSRC)/rpt_comm.hip $(CSRC)/rpt_lights.hip $(CSRC)/rpt_bvh.hip $(CSRC)/rpt_denoise.hip $(CSRC)/rpt_moments.hip $(CSRC)/rpt_adaptive.hip $(CSRC)/rpt_models.hip $(CSRC)/rpt_volumes.hip $(CSRC)/rpt_punctual.hip $(CSRC)/rpt_lens.hip $(CSRC)/rpt_debug.hip
HIP_OBJS  := $(patsubst $(CSRC)/%.hip,build/%.o,$(HIP_SRCS))
HIP_DEPS  := $(wildcard $(CSRC)/*.h) $(wildcard $(CSRC)/*.hip) $(wildcard include/rpt/*.h)

CXXFLAGS_COMMON := -std=c++20 -O2 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unknown-pragmas
# -mfma only makes the EXPLICIT __builtin_fma of rpt_math.h a single instruction;
# implicit contraction stays off.
ORACLE_FLAGS := $(CXXFLAGS_COMMON) -mfma -msse4.1 -pthread
HIPFLAGS := --offload-arch=gfx950 -std=c++20 -O3 -fPIC -ffp-contract=off -fno-fast-math \
            -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero \
            -Wall -Wno-unused-function -fno-slp-vectorize
# -fno-slp-vectorize: the packed f32 operations the SLP vectorizer forms issue in the time of two plain ones on gfx950 and cost v_mov
# shuffles and registers (profiles/r03_slp.txt)

all: host oracle hip fake_rccl models_oracle lens_oracle volume_oracle lights_oracle

host: $(LIBDIR)/librpt_host.so
oracle: oracle/liboracle.so oracle/liboracle_libm.so
hip: $(LIBDIR)/librpt_hip.so

$(LIBDIR)/librpt_host.so: $(HOST_SRCS) $(CSRC)/host/host_internal.h $(CSRC)/rpt_math.h include/rpt/rpt_host.h include/rpt/rpt.h include/rpt/shared_structs.h
	@mkdir -p $(LIBDIR)
	$(CXX) $(CXXFLAGS_COMMON) -shared -o $@ $(HOST_SRCS) -lz -ldl -pthread

oracle/liboracle.so: oracle/rpt_oracle.cpp oracle/bvh_oracle.cpp $(CSRC)/rpt_math.h $(CSRC)/rpt_fastdiv.h $(CSRC)/rpt_rcp.h $(CSRC)/rpt_math_consts.h include/rpt/shared_structs.h
	$(CXX) $(ORACLE_FLAGS) -shared -o $@ oracle/rpt_oracle.cpp oracle/bvh_oracle.cpp

oracle/liboracle_libm.so: oracle/rpt_oracle.cpp oracle/bvh_oracle.cpp $(CSRC)/rpt_math.h $(CSRC)/rpt_fastdiv.h $(CSRC)/rpt_rcp.h $(CSRC)/rpt_math_consts.h include/rpt/shared_structs.h
	$(CXX) $(ORACLE_FLAGS) -DORACLE_USE_LIBM -shared -o $@ oracle/rpt_oracle.cpp oracle/bvh_oracle.cpp -lm

# test infrastructure: the restatement of trace_pixel with the model switch (tests/models_oracle/models_oracle.cpp includes oracle/rpt_oracle.cpp
# textually); -Bsymbolic: its copy of the oracle's exported names binds to itself, whichever library a process loaded first.  Built BESIDE the oracle, not
# beside its source: a build product under tests/ is lost when another commit's tests/ is put over a built tree, and the tests of that commit then fail
models_oracle: oracle/libmodels_oracle.so
oracle/libmodels_oracle.so: tests/models_oracle/models_oracle.cpp tests/lens_oracle/lens_camera.h oracle/rpt_oracle.cpp $(CSRC)/rpt_math.h $(CSRC)/rpt_fastdiv.h $(CSRC)/rpt_rcp.h $(CSRC)/rpt_math_consts.h include/rpt/shared_structs.h
	$(CXX) $(ORACLE_FLAGS) -shared -Wl,-Bsymbolic -o $@ tests/models_oracle/models_oracle.cpp

# test infrastructure: the restatement of trace_pixel with the thin-lens camera of rpt_set_camera_lens in place of lib.rs:38-51 (tests/lens_oracle/lens_oracle.cpp
# includes oracle/rpt_oracle.cpp textually), built like models_oracle
lens_oracle: oracle/liblens_oracle.so
oracle/liblens_oracle.so: tests/lens_oracle/lens_oracle.cpp tests/lens_oracle/lens_camera.h oracle/rpt_oracle.cpp $(CSRC)/rpt_math.h $(CSRC)/rpt_fastdiv.h $(CSRC)/rpt_rcp.h $(CSRC)/rpt_math_consts.h include/rpt/shared_structs.h
	$(CXX) $(ORACLE_FLAGS) -shared -Wl,-Bsymbolic -o $@ tests/lens_oracle/lens_oracle.cpp

# test infrastructure: the restatement of trace_pixel with the model switch, the lens and the absorption rule of rpt_set_material_volumes
# (tests/volume_oracle/volume_oracle.cpp includes oracle/rpt_oracle.cpp textually), built like models_oracle
volume_oracle: oracle/libvolume_oracle.so
oracle/libvolume_oracle.so: tests/volume_oracle/volume_oracle.cpp tests/lens_oracle/lens_camera.h oracle/rpt_oracle.cpp $(CSRC)/rpt_math.h $(CSRC)/rpt_fastdiv.h $(CSRC)/rpt_rcp.h $(CSRC)/rpt_math_consts.h include/rpt/shared_structs.h
	$(CXX) $(ORACLE_FLAGS) -shared -Wl,-Bsymbolic -o $@ tests/volume_oracle/volume_oracle.cpp

# test infrastructure: the volume restatement with the punctual lights of rpt_set_punctual_lights (tests/lights_oracle/lights_oracle.cpp includes
# oracle/rpt_oracle.cpp textually), built like volume_oracle
lights_oracle: oracle/liblights_oracle.so
oracle/liblights_oracle.so: tests/lights_oracle/lights_oracle.cpp tests/lens_oracle/lens_camera.h oracle/rpt_oracle.cpp $(CSRC)/rpt_math.h $(CSRC)/rpt_fastdiv.h $(CSRC)/rpt_rcp.h $(CSRC)/rpt_math_consts.h include/rpt/shared_structs.h
	$(CXX) $(ORACLE_FLAGS) -shared -Wl,-Bsymbolic -o $@ tests/lights_oracle/lights_oracle.cpp

# the fingerprint of the device-side sources is compiled in (rpt_build_fingerprint): bench.py reports PMC-derived figures only for the
# sources the LOADED library was built from, and says so when the library is older than the source tree
# one object per translation unit, built in PARALLEL (the recipe below re-invokes make with one job per unit): the walk kernels (rpt_traverse.hip)
# and the shade / sky kernels (rpt_hip.hip) take longest and bound the build
build/%.o: $(CSRC)/%.hip $(HIP_DEPS) tools/source_fingerprint.py Makefile
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -DRPT_BUILD_FINGERPRINT=\"$$(python3 tools/source_fingerprint.py)\" -c -o $@ $<

$(LIBDIR)/librpt_hip.so: $(HIP_SRCS) $(HIP_DEPS) tools/source_fingerprint.py Makefile
	@mkdir -p $(LIBDIR)
	$(MAKE) -j$(words $(HIP_SRCS)) $(HIP_OBJS)
	$(HIPCC) --offload-arch=gfx950 -fPIC -shared -o $@ $(HIP_OBJS) -ldl

# test infrastructure: a stand-in for RCCL's point-to-point calls over shared memory, so that N PROCESSES on a one-GPU test box run
# the product's gather unchanged (tests/test_gpu_multiprocess.py; selected with RPT_RCCL_LIBRARY, never linked by the product)
fake_rccl: tests/fake_rccl/librccl_fake.so
tests/fake_rccl/librccl_fake.so: tests/fake_rccl/fake_rccl.cpp
	$(HIPCC) -x c++ -std=c++17 -O2 -fPIC -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -shared -o $@ $< -L/opt/rocm/lib -lamdhip64 -lrt -pthread

clean:
	rm -f $(LIBDIR)/*.so oracle/*.so tests/fake_rccl/*.so

.PHONY: all host oracle hip fake_rccl models_oracle lens_oracle volume_oracle lights_oracle clean
