# Build recipe for the native pieces.  `make` builds the product library (HIP, gfx950).
# `make hostcheck` builds the CPU debug harness of the per-ray core used by tests only.
# `make poolcheck poolcheck-tsan` build the host check of the block cache (trc_pool.h: one cache, under one policy for device memory
# and another for pinned host memory) with the address / undefined-behaviour sanitizers and with the thread sanitizer.
# `make scenecheck` builds the host check of a scene's host arithmetic (trc_scene_host.h) with the same sanitizers.
# `make sourcecheck sourcecheck-tsan` build the host check of the tabulated sources' host side (trc_source_host.h) with both.
ROOT := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
HIPCC ?= hipcc
CXX ?= g++
ARCH ?= gfx950

LIB := $(ROOT)tracer_amd/lib/libtracer_amd.so
CSRC := $(ROOT)tracer_amd/csrc
# five translation units: the engines (trc_kernels.hip, which includes trc_stream.inc), the class-split shading kernels of the
# streaming engine (trc_shade.hip), the scene's part of the C-ABI (trc_scene.hip), the histograms of captured hits with their entry
# points (trc_hithist.hip), and the entry points that take no scene with their kernels (trc_protocol.hip).  `make -j4` compiles
# them side by side.
UNITS := trc_kernels trc_shade trc_scene trc_hithist trc_protocol
SRCS := $(UNITS:%=$(CSRC)/%.hip)
OBJDIR := $(ROOT)build/obj
OBJS := $(UNITS:%=$(OBJDIR)/%.o)
HDR := $(CSRC)/trc_host.h $(CSRC)/trc_scene.h $(CSRC)/trc_source_host.h $(CSRC)/trc_core.h $(CSRC)/trc_bounds.h $(CSRC)/trc_footprint.h $(CSRC)/trc_forms.h $(CSRC)/trc_device.h $(CSRC)/trc_stream.inc $(CSRC)/trc_mega.inc $(CSRC)/trc_hithist.h $(CSRC)/trc_pool.h $(CSRC)/trc_scene_host.h $(ROOT)include/tracer_amd.h

HOSTCHECK := $(ROOT)tests/hostcheck/libtrc_hostcheck.so
HOSTCHECK_SRC := $(ROOT)tests/hostcheck/hostcheck.cpp
SPECCHECK := $(ROOT)tests/hostcheck/libtrc_spectrum_check.so
SPECCHECK_SRC := $(ROOT)tests/hostcheck/spectrum_check.cpp
SUNCHECK := $(ROOT)tests/hostcheck/libtrc_sunshape_check.so
SUNCHECK_SRC := $(ROOT)tests/hostcheck/sunshape_check.cpp
LAMPCHECK := $(ROOT)tests/hostcheck/libtrc_lamp_check.so
LAMPCHECK_SRC := $(ROOT)tests/hostcheck/lamp_check.cpp
FMCHECK := $(ROOT)tests/hostcheck/libtrc_fluxmap_check.so
FMCHECK_SRC := $(ROOT)tests/hostcheck/fluxmap_check.cpp
HHCHECK := $(ROOT)tests/hostcheck/libtrc_hithist_check.so
HHCHECK_SRC := $(ROOT)tests/hostcheck/hithist_check.cpp
HHXCHECK := $(ROOT)tests/hostcheck/libtrc_hithist_x_check.so
HHXCHECK_SRC := $(ROOT)tests/hostcheck/hithist_x_check.cpp
THERMCHECK := $(ROOT)tests/hostcheck/libtrc_thermal_check.so
THERMCHECK_EXE := $(ROOT)tests/hostcheck/thermal_check
THERMCHECK_SRC := $(ROOT)tests/hostcheck/thermal_check.cpp

UMASKCHECK := $(ROOT)tests/umaskcheck/libtrc_umask_check.so
UMASKCHECK_EXE := $(ROOT)tests/umaskcheck/umask_check
UMASKCHECK_SRC := $(ROOT)tests/umaskcheck/umask_check.cpp

all: $(LIB)

# -ffp-contract=off: a*b+c is rounded twice, as NumPy rounds it in the reference.  Fused, the same formula rounds differently in
# each kernel it is inlined into, and the forms of the engine end ~1e-7 of the rays on different surfaces;
# it costs 0.8 % on the bench.  fma() where it is written stays an fma.
FPFLAGS := -ffp-contract=off

HIPFLAGS := -O3 -std=c++17 --offload-arch=$(ARCH) -munsafe-fp-atomics $(FPFLAGS) -fPIC -Wno-unused-result

# No machine-level loop-invariant code motion.  The kernels are grid-stride loops around chains of float64 library code
# (logarithm, sine / cosine, tangent, arc cosine, square roots and divisions), and the pass moves the materialisation of every
# constant of those chains in front of the loop, where each then holds two registers for the whole kernel: the lean shading
# kernels 170 / 241 registers with it, 94 / 116 without; k_s_shade 243 -> 131, k_s_fresh 168 -> 95, k_s_bounce 128 + 180 bytes of
# scratch -> 119, k_trace_coop 256 + 408 bytes -> 165, k_ord_bounce 166 -> 121 (build/*.resources.txt, `make asm`).
# Measured (profiles/README.md): NSTTF +3 %, dish +4 %, cavity +9 %, the megakernel on the dish +17 %.
# One rule for every unit, under UNIT_FLAGS; SHADE_FLAGS is what trc_shade.hip alone is compiled under (the same today).
KERNELS_FLAGS := -mllvm -disable-machine-licm
SHADE_FLAGS := $(KERNELS_FLAGS)
UNIT_FLAGS = $(KERNELS_FLAGS)
$(OBJDIR)/trc_shade.o: UNIT_FLAGS = $(SHADE_FLAGS)

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDR)
	mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(UNIT_FLAGS) -c -o $@ $<

$(LIB): $(OBJS)
	mkdir -p $(dir $(LIB))
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared -o $@ $(OBJS)

MATCHECK := $(ROOT)tests/hostcheck/libtrc_material_check.so
MATCHECK_SRC := $(ROOT)tests/hostcheck/material_check.cpp

hostcheck: $(HOSTCHECK) $(SPECCHECK) $(SUNCHECK) $(FMCHECK) $(MATCHECK) $(LAMPCHECK) $(HHCHECK) $(HHXCHECK) $(THERMCHECK)

# the tabulated materials' lookup of the per-ray core, host-compiled for its tests
$(MATCHECK): $(MATCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(MATCHECK_SRC)

$(HOSTCHECK): $(HOSTCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(HOSTCHECK_SRC)

# the source-spectrum sampler of the per-ray core, host-compiled for its tests
$(SPECCHECK): $(SPECCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(SPECCHECK_SRC)

# the tabulated-sunshape sampler and sources of the per-ray core, host-compiled for their tests
$(SUNCHECK): $(SUNCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(SUNCHECK_SRC)

# the arc-lamp sources of the per-ray core and the decisions for their kinds, host-compiled for their tests
$(LAMPCHECK): $(LAMPCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(LAMPCHECK_SRC)

# the thermal emitters of the per-ray core -- the emittance table's packing, its exact sampler, the shapes -- host-compiled for their
# tests; and the same source as a program of its own (thermalcheck), built with the sanitizers, that runs the sampler over a grid of
# uniforms and is run by tests/test_thermal_sources_host.py
$(THERMCHECK): $(THERMCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(THERMCHECK_SRC)

thermalcheck: $(THERMCHECK_EXE)

$(THERMCHECK_EXE): $(THERMCHECK_SRC) $(HDR)
	$(CXX) -O1 -g -std=c++17 $(FPFLAGS) $(SPLIT_SAN) -DTHERMAL_CHECK_MAIN -o $@ $(THERMCHECK_SRC)

# the flux-map charts and bin index of the per-ray core, host-compiled for their tests
$(FMCHECK): $(FMCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(FMCHECK_SRC)

# the histogram of captured hits -- its per-hit function, its LDS decision and its pass as a host loop -- host-compiled for their tests
$(HHCHECK): $(HHCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(HHCHECK_SRC)

# the spectral histogram of captured hits -- where its kernel keeps its bins, and its pass as a host loop, slice by slice -- host-compiled
# for their tests
$(HHXCHECK): $(HHXCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(HHXCHECK_SRC)

# the footprint map's mask over the uniforms against brute force, host-compiled: a library for its test, and the same as a program
# (umaskcheck-exe; SAN="-fsanitize=address,undefined" builds it for a sanitizer run)
umaskcheck: $(UMASKCHECK)
umaskcheck-exe: $(UMASKCHECK_EXE)

$(UMASKCHECK): $(UMASKCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(UMASKCHECK_SRC)

$(UMASKCHECK_EXE): $(UMASKCHECK_SRC) $(HDR)
	$(CXX) -O2 -g -std=c++17 $(FPFLAGS) $(SAN) -DUMASK_CHECK_MAIN -o $@ $(UMASKCHECK_SRC)

# the clear cones of the LDS-sized grid (trc_clear_build: trc_bounds.h) against brute force over the boxes, host-compiled: a library
# for tests/test_clear_cones_host.py, and the same as a program of its own, built with the sanitizers, that the test runs as a child
CLEARCHECK := $(ROOT)tests/clearcheck/libtrc_clear_check.so
CLEARCHECK_EXE := $(ROOT)tests/clearcheck/clear_check
CLEARCHECK_SRC := $(ROOT)tests/clearcheck/clear_check.cpp
clearcheck: $(CLEARCHECK) $(CLEARCHECK_EXE)

$(CLEARCHECK): $(CLEARCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(CLEARCHECK_SRC)

$(CLEARCHECK_EXE): $(CLEARCHECK_SRC) $(HDR)
	$(CXX) -O1 -g -std=c++17 $(FPFLAGS) $(SPLIT_SAN) -DCLEAR_CHECK_MAIN -o $@ $(CLEARCHECK_SRC)

# whether the shading kernels finish the next segment of the rays inside their clear cones (trc_stream_form_ahead: trc_forms.h), on the
# fact blocks of the host check: a library for tests/test_finish_ahead_host.py
AHEADCHECK := $(ROOT)tests/aheadcheck/libtrc_ahead_check.so
AHEADCHECK_SRC := $(ROOT)tests/aheadcheck/ahead_check.cpp
aheadcheck: $(AHEADCHECK)

$(AHEADCHECK): $(AHEADCHECK_SRC) $(HOSTCHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(AHEADCHECK_SRC)

# the room of a streaming call whose optics split rays (trc_split_room_need, trc_split_grow: trc_bounds.h) on a grid of inputs: a
# program of its own, built with the sanitizers and run by tests/test_split_cases_host.py
SPLITCHECK_EXE := $(ROOT)tests/splitcheck/split_check
SPLITCHECK_SRC := $(ROOT)tests/splitcheck/split_check.cpp
SPLIT_SAN ?= -fsanitize=address,undefined -fno-sanitize-recover=undefined
splitcheck: $(SPLITCHECK_EXE)

$(SPLITCHECK_EXE): $(SPLITCHECK_SRC) $(HDR)
	$(CXX) -O1 -g -std=c++17 $(FPFLAGS) $(SPLIT_SAN) -o $@ $(SPLITCHECK_SRC)

# what k_s_shade_p rests on -- trc_interp2_at against trc_interp2 bit for bit, the ids and the LDS decision of its family
# (trc_forms.h) -- as a program of its own, built with the sanitizers and run by tests/test_poly_source_host.py
POLYCHECK_EXE := $(ROOT)tests/polycheck/poly_check
POLYCHECK_SRC := $(ROOT)tests/polycheck/poly_check.cpp
polycheck: $(POLYCHECK_EXE)

$(POLYCHECK_EXE): $(POLYCHECK_SRC) $(HDR)
	$(CXX) -O1 -g -std=c++17 $(FPFLAGS) $(SPLIT_SAN) -o $@ $(POLYCHECK_SRC)

# the block cache behind device and pinned memory (trc_pool.h) through a fake backend: its classes, caps, eviction order, retry and
# device key, and its books after eight threads have used it.  Two programs of their own, run by tests/test_pool_host.py
POOLCHECK_EXE := $(ROOT)tests/poolcheck/pool_check
POOLCHECK_TSAN_EXE := $(ROOT)tests/poolcheck/pool_check_tsan
POOLCHECK_SRC := $(ROOT)tests/poolcheck/pool_check.cpp
poolcheck: $(POOLCHECK_EXE)
poolcheck-tsan: $(POOLCHECK_TSAN_EXE)

$(POOLCHECK_EXE): $(POOLCHECK_SRC) $(CSRC)/trc_pool.h
	$(CXX) -O1 -g -std=c++17 $(SPLIT_SAN) -pthread -o $@ $(POOLCHECK_SRC)

$(POOLCHECK_TSAN_EXE): $(POOLCHECK_SRC) $(CSRC)/trc_pool.h
	$(CXX) -O1 -g -std=c++17 -fsanitize=thread -pthread -o $@ $(POOLCHECK_SRC)

# the host side of a scene (trc_scene_host.h): the Kd-tree validation on malformed trees, its packing, the tally layout and the build
# order of the search tables.  A program of its own, built with the sanitizers and run by tests/test_scene_host.py
SCENECHECK_EXE := $(ROOT)tests/scenecheck/scene_check
SCENECHECK_SRC := $(ROOT)tests/scenecheck/scene_check.cpp
scenecheck: $(SCENECHECK_EXE)

$(SCENECHECK_EXE): $(SCENECHECK_SRC) $(HDR)
	$(CXX) -O1 -g -std=c++17 $(FPFLAGS) $(SPLIT_SAN) -o $@ $(SCENECHECK_SRC)

# the host side of the tabulated sources (trc_source_host.h): the one table check on bad tables by status and message, the packing
# bit for bit, the id registry (in order, to exhaustion, under eight threads) and the descriptor arithmetic.  Two programs of their
# own, run by tests/test_source_tables_host.py, and the check-and-pack functions as a library for the same test.  (The library is
# built by `sourcecheck`, not by `hostcheck`: what `hostcheck` builds needs nothing outside tests/hostcheck.)
SOURCECHECK_EXE := $(ROOT)tests/sourcecheck/source_check
SOURCECHECK_TSAN_EXE := $(ROOT)tests/sourcecheck/source_check_tsan
SOURCECHECK_LIB := $(ROOT)tests/sourcecheck/libtrc_source_check.so
SOURCECHECK_SRC := $(ROOT)tests/sourcecheck/source_check.cpp
sourcecheck: $(SOURCECHECK_EXE) $(SOURCECHECK_LIB)
sourcecheck-tsan: $(SOURCECHECK_TSAN_EXE)

$(SOURCECHECK_EXE): $(SOURCECHECK_SRC) $(HDR)
	$(CXX) -O1 -g -std=c++17 $(FPFLAGS) $(SPLIT_SAN) -pthread -DSOURCE_CHECK_MAIN -o $@ $(SOURCECHECK_SRC)

$(SOURCECHECK_TSAN_EXE): $(SOURCECHECK_SRC) $(HDR)
	$(CXX) -O1 -g -std=c++17 $(FPFLAGS) -fsanitize=thread -pthread -DSOURCE_CHECK_MAIN -o $@ $(SOURCECHECK_SRC)

$(SOURCECHECK_LIB): $(SOURCECHECK_SRC) $(HDR)
	$(CXX) -O2 -std=c++17 -fPIC -shared $(FPFLAGS) -o $@ $(SOURCECHECK_SRC)

# assembly listings with the registers, scratch and occupancy of every kernel (build/*.s, build/*.resources.txt)
asm: $(SRCS) $(HDR)
	mkdir -p $(ROOT)build
	for f in $(UNITS); do \
		fl="$(KERNELS_FLAGS)"; [ $$f = trc_shade ] && fl="$(SHADE_FLAGS)"; \
		$(HIPCC) $(HIPFLAGS) $$fl -S --cuda-device-only -Rpass-analysis=kernel-resource-usage \
			-o $(ROOT)build/$$f.s $(CSRC)/$$f.hip 2> $(ROOT)build/$$f.resources.txt || exit 1; done

asm-shade: $(CSRC)/trc_shade.hip $(HDR)
	mkdir -p $(ROOT)build
	$(HIPCC) $(HIPFLAGS) $(SHADE_FLAGS) -S --cuda-device-only -Rpass-analysis=kernel-resource-usage \
		-o $(ROOT)build/trc_shade.s $(CSRC)/trc_shade.hip 2> $(ROOT)build/trc_shade.resources.txt

clean:
	rm -f $(LIB) $(HOSTCHECK) $(SPECCHECK) $(SUNCHECK) $(FMCHECK) $(MATCHECK) $(LAMPCHECK) $(HHCHECK) $(HHXCHECK) $(THERMCHECK) $(THERMCHECK_EXE) $(SOURCECHECK_LIB)

.PHONY: all hostcheck thermalcheck umaskcheck umaskcheck-exe clearcheck aheadcheck splitcheck polycheck poolcheck poolcheck-tsan scenecheck sourcecheck sourcecheck-tsan asm asm-shade clean
