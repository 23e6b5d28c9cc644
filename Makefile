# Builds (all in-tree so the .so files travel to the GPU box with the snapshot):
#   intent-mpc_amd/lib/libimpc_qp.so      product: HIP kernels (gfx950) + C-ABI + host symbolic
#                                         analysis + MPC->QP builder; one translation unit per
#                                         module of intent-mpc_amd/csrc (*.hip, *.cpp), each rebuilt
#                                         only when a file it includes changes
#   oracle/build/libosqp_oracle.so        test oracle: C restatement of OSQP 0.6.2 (gcc)
#   tests/native/build/libimpc_core_cpu.so test-only CPU build of admm_core.hpp (debug harness)
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CC      ?= gcc
ROOT    := $(abspath $(dir $(lastword $(MAKEFILE_LIST))))
CSRC    := $(ROOT)/intent-mpc_amd/csrc
LIBDIR  := $(ROOT)/intent-mpc_amd/lib
ORADIR  := $(ROOT)/oracle/build
HARNDIR := $(ROOT)/tests/native/build

# -fno-unroll-loops: the structured kernel's runtime-bound loops (stage recursions, gathers,
# Cholesky) are unrolled by hand where it pays; compiler unrolling of the rest only raises
# register pressure past the 2-waves-per-SIMD budget (measured).
HIPFLAGS  := -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function -fno-unroll-loops
HOSTFLAGS := -O2 -std=c++17 -fPIC -ffp-contract=off -Wall
# RCCL (multi-GPU cost all-gather, include/impc_comm.h), from the same ROCm as the HIP runtime
LDLIBS    := -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

# build identity baked into the library (impc_build_id, csrc/build_id.cpp): every source compiled into
# it + the flags.  Only the id unit takes it, so only the id unit is rebuilt for every source change.
SRCS    := $(sort $(wildcard $(CSRC)/*.hip $(CSRC)/*.hpp $(CSRC)/*.cpp $(ROOT)/include/*.h))
BUILD_ID := src-$(shell cat $(SRCS) | { cat; echo '$(HIPFLAGS) $(HOSTFLAGS)'; } | sha256sum | cut -c1-16)
GIT_REV := $(shell git -C $(ROOT) rev-parse --short HEAD 2>/dev/null || echo unknown)
IDFLAGS  = -DIMPC_BUILD_ID='"$(BUILD_ID)$(1)"' -DIMPC_GIT_REV='"$(GIT_REV)"'

# the library: one object per csrc/*.hip (device + host) and per csrc/*.cpp (host).  SOLVER is the
# structured and generic solver's unit (minutes to compile); REST is every other object.
OBJS    := $(patsubst $(CSRC)/%,$(LIBDIR)/%.o,$(basename $(filter %.hip %.cpp,$(SRCS))))
SOLVER  := $(LIBDIR)/impc_qp.o
REST    := $(filter-out $(SOLVER) $(LIBDIR)/build_id.o,$(OBJS))
LINK     = $(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $^ -o $@ $(LDLIBS)

LIB     := $(LIBDIR)/libimpc_qp.so
PROFLIB := $(LIBDIR)/libimpc_qp_prof.so
ORACLE  := $(ORADIR)/libosqp_oracle.so
HARNESS := $(HARNDIR)/libimpc_core_cpu.so
EMU     := $(HARNDIR)/libwave_emu.so
EMU64   := $(HARNDIR)/libwave_emu64.so
SHIMT   := $(HARNDIR)/shim_test
REPLANX := $(HARNDIR)/replan_example
DETECTH := $(HARNDIR)/libdetect_harness.so
EXECH   := $(HARNDIR)/libexec_harness.so
MFMODEL := $(HARNDIR)/sweep_mfma_model
STMODEL := $(HARNDIR)/sweep_store_model
CLUSTH  := $(HARNDIR)/libcluster_harness.so

.PHONY: all lib oracle harness prof variant clean
all: lib oracle harness
lib: $(LIB)
oracle: $(ORACLE)
harness: $(HARNESS) $(EMU) $(EMU64) $(SHIMT) $(REPLANX) $(DETECTH) $(EXECH) $(MFMODEL) $(STMODEL) $(CLUSTH)

# each unit depends on what it includes, as the compiler reports it (lib/*.d)
$(LIBDIR)/%.o: $(CSRC)/%.hip
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c $< -o $@
$(LIBDIR)/%.o: $(CSRC)/%.cpp
	@mkdir -p $(LIBDIR)
	$(CXX) $(HOSTFLAGS) -MMD -MP -c $< -o $@
-include $(wildcard $(LIBDIR)/*.d)

# the id unit, per library: build_id.o for the product, build_id_<name>.o with the id suffix -<name>
$(LIBDIR)/build_id.o: $(CSRC)/build_id.cpp $(SRCS)
	@mkdir -p $(LIBDIR)
	$(CXX) $(HOSTFLAGS) $(call IDFLAGS,) -c $< -o $@
$(LIBDIR)/build_id_%.o: $(CSRC)/build_id.cpp $(SRCS)
	@mkdir -p $(LIBDIR)
	$(CXX) $(HOSTFLAGS) $(call IDFLAGS,-$*) -c $< -o $@

$(LIB): $(SOLVER) $(LIBDIR)/build_id.o $(REST)
	$(LINK)

# section-profiling variant of the library (tools/section_profile.py; never the product): the solver
# unit with the extra define, every other object as it is
prof: $(PROFLIB)
$(LIBDIR)/impc_qp_prof.o: $(CSRC)/impc_qp.hip
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -MMD -MP -DIMPC_SECTION_PROF -c $< -o $@
$(PROFLIB): $(LIBDIR)/impc_qp_prof.o $(LIBDIR)/build_id_prof.o $(REST)
	$(LINK)

# kernel experiments (tools/ only): make variant V=name DEFS="-DX=1" -> lib/libimpc_qp_<name>.so,
# selected at run time with IMPC_LIB_VARIANT=<name>; the solver unit is compiled on every call
variant: $(LIBDIR)/build_id_$(V).o $(REST)
	$(HIPCC) $(HIPFLAGS) $(DEFS) -c $(CSRC)/impc_qp.hip -o $(LIBDIR)/impc_qp_$(V).o
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $(LIBDIR)/impc_qp_$(V).o $^ -o $(LIBDIR)/libimpc_qp_$(V).so $(LDLIBS)

$(ORACLE): $(ROOT)/oracle/osqp_oracle.c
	@mkdir -p $(ORADIR)
	$(CC) -O2 -fPIC -shared -std=c11 -ffp-contract=off -Wall -o $@ $< -lm -lpthread

$(HARNESS): $(ROOT)/tests/native/core_harness.cpp $(CSRC)/admm_core.hpp $(CSRC)/symbolic.cpp $(CSRC)/symbolic.hpp
	@mkdir -p $(HARNDIR)
	$(HIPCC) -x hip -O2 -std=c++17 -fPIC -shared --offload-arch=$(ARCH) -ffp-contract=off \
		$(ROOT)/tests/native/core_harness.cpp -x c++ $(CSRC)/symbolic.cpp -o $@

$(EMU): $(ROOT)/tests/native/wave_emu.cpp $(CSRC)/mpc_wave.hpp $(CSRC)/admm_core.hpp $(CSRC)/mpc_structure.cpp \
		$(CSRC)/mpc_structure.hpp $(CSRC)/sweep_mfma_map.hpp
	@mkdir -p $(HARNDIR)
	$(HIPCC) -x hip --offload-host-only -std=c++20 -O2 -fPIC -shared -ffp-contract=off \
		$(ROOT)/tests/native/wave_emu.cpp -x c++ $(CSRC)/mpc_structure.cpp -o $@

# the one-QP-per-wavefront team shape (64 lanes, four variables per lane) in the same emulation
$(EMU64): $(ROOT)/tests/native/wave_emu.cpp $(CSRC)/mpc_wave.hpp $(CSRC)/admm_core.hpp $(CSRC)/mpc_structure.cpp \
		$(CSRC)/mpc_structure.hpp $(CSRC)/sweep_mfma_map.hpp
	@mkdir -p $(HARNDIR)
	$(HIPCC) -x hip --offload-host-only -std=c++20 -O2 -fPIC -shared -ffp-contract=off -DEMU_NL=64 \
		$(ROOT)/tests/native/wave_emu.cpp -x c++ $(CSRC)/mpc_structure.cpp -o $@

# OsqpEigen shim driver (test-only Eigen stand-in; links the product library)
$(SHIMT): $(ROOT)/tests/native/shim_test.cpp $(ROOT)/include/OsqpEigen/OsqpEigen.h $(LIB)
	@mkdir -p $(HARNDIR)
	$(CXX) -O2 -std=c++17 -Wall -I$(ROOT)/tests/native/mock_eigen -I$(ROOT)/include $< -L$(LIBDIR) -limpc_qp \
		-Wl,-rpath,'$$ORIGIN/../../../intent-mpc_amd/lib' -o $@

# batched makePlanWithPred over the C-ABI only (C++ integration example, driven by the tests)
$(REPLANX): $(ROOT)/tests/native/replan_example.cpp $(ROOT)/include/impc_qp.h $(ROOT)/include/impc_mpc.h \
		$(ROOT)/include/impc_replan.h $(LIB)
	@mkdir -p $(HARNDIR)
	$(CXX) -O2 -std=c++17 -Wall -I$(ROOT)/include $< -L$(LIBDIR) -limpc_qp \
		-Wl,-rpath,'$$ORIGIN/../../../intent-mpc_amd/lib' -o $@

# the range gate's predicate (csrc/detect_gate.hpp) compiled for the host
$(DETECTH): $(ROOT)/tests/native/detect_harness.cpp $(CSRC)/detect_gate.hpp
	@mkdir -p $(HARNDIR)
	$(HIPCC) -x hip --offload-host-only -std=c++17 -O2 -fPIC -shared -ffp-contract=off $< -o $@

# the plan getters, tracking target and collision tests (csrc/plan_exec.hpp) compiled for the host
$(EXECH): $(ROOT)/tests/native/exec_harness.cpp $(CSRC)/plan_exec.hpp $(ROOT)/include/impc_exec.h \
		$(ROOT)/include/impc_replan.h $(ROOT)/include/impc_predict.h
	@mkdir -p $(HARNDIR)
	$(HIPCC) -x hip --offload-host-only -std=c++17 -O2 -fPIC -shared -ffp-contract=off $< -o $@

# the serial form of the static-obstacle producer (csrc/cluster.hpp) compiled for the host
$(CLUSTH): $(ROOT)/tests/native/cluster_harness.cpp $(CSRC)/cluster.hpp $(ROOT)/include/impc_cluster.h \
		$(ROOT)/include/impc_predict.h
	@mkdir -p $(HARNDIR)
	$(HIPCC) -x hip --offload-host-only -std=c++17 -O2 -fPIC -shared -ffp-contract=off -Wall -Wno-unused-function $< -o $@ -lpthread

# host model of the stage recursions on the FP64 matrix instruction against a plain loop (stand-alone,
# host only; SAN="-fsanitize=address,undefined" for a checked build)
$(MFMODEL): $(ROOT)/tests/native/sweep_mfma_model.cpp $(CSRC)/sweep_mfma_map.hpp
	@mkdir -p $(HARNDIR)
	$(CXX) -O1 -g -std=c++17 -Wall -ffp-contract=off $(SAN) $< -o $@

# host model of the sweeps' capture registers and their early stores (stand-alone, host only; SAN as above)
$(STMODEL): $(ROOT)/tests/native/sweep_store_model.cpp $(CSRC)/sweep_mfma_map.hpp
	@mkdir -p $(HARNDIR)
	$(CXX) -O1 -g -std=c++17 -Wall -ffp-contract=off $(SAN) $< -o $@

clean:
	rm -rf $(LIBDIR) $(ORADIR) $(HARNDIR)
