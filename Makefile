# vame -- MI355X affine-ME engine.  `make` builds everything in-tree:
#   vvc-affine-gpu_amd/lib/libvame.so   HIP kernels (gfx950) + C ABI (include/vame.h)
#   vvc-affine-gpu_amd/bin/vame         C++ CLI, drop-in for the reference's ./main
#   oracle/libvame_oracle.so            CPU restatement (tests / CPU baseline only)
#   oracle/_ref/*                       reference kernels + harness (only where /root/reference exists)

HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
PKG     := vvc-affine-gpu_amd
CSRC    := $(PKG)/csrc
LIBDIR  := $(PKG)/lib
BINDIR  := $(PKG)/bin
# -ffp-contract=off: the FP64 solve must round exactly like the reference
# (explicit fma where OpenCL's FP_CONTRACT fuses); integer paths are unaffected.
# -disable-machine-licm: the quadrant kernel's task loop (several tasks per
# workgroup) made MachineLICM hoist constants and lane addresses out of it and
# spill registers for them (16-48 B/lane, their writes reaching HBM); without
# it every kernel runs at zero scratch.
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function \
            -mllvm -disable-machine-licm
# SimplifyCFG's sinking (and, for the 2-CP-only kernels, hoisting) of code
# common to both sides of a branch stretched live ranges across the kernels'
# per-item and per-kind branches into spill slots: without it the kernels of
# the engine's unit drop to 0-32 B of scratch per lane and the 2-CP-only ones
# (vame_kernels_2cp.hip) from 76-84 B to 0-40 B; c2 -2.3 %, c3 / c4 -0.8 %
# (profiles/r06_quad2_ab.txt, seventh and eighth A/B).
# Uniform branches left unstructurized (the per-item and per-kind branches
# are wave-uniform): scratch 0 in the quadrant kernels, c2 -1.1 %, c4 -0.6 %
# (ninth A/B).
KFLAGS     := -mllvm -simplifycfg-sink-common=false -mllvm -structurizecfg-skip-uniform-regions=true
KFLAGS_2CP := -mllvm -simplifycfg-sink-common=false -mllvm -simplifycfg-hoist-common=false \
              -mllvm -structurizecfg-skip-uniform-regions=true

# The library's units, one word each: <object tag>=<source>[=<variable with its
# own flags>].  Everything below -- build_lib, resource-usage, the
# dependencies -- goes over this list: a new unit is one word here.
UNITS := engine=vame_engine.hip=KFLAGS 2cp=vame_kernels_2cp.hip=KFLAGS_2CP stages=vame_stages.hip \
         pack=vame_pack.hip=KFLAGS templates=vame_templates.cpp mc=vame_mc.hip \
         partition=vame_partition.hip bipred=vame_bipred.hip birefine=vame_birefine.hip \
         seed=vame_seed.hip search=vame_search.hip \
         birefine_p=vame_birefine_p.hip search_p=vame_search_p.hip \
         hostlogic=vame_hostlogic.cpp io=vame_io.cpp
unit_tag   = $(word 1,$(subst =, ,$(1)))
unit_src   = $(CSRC)/$(word 2,$(subst =, ,$(1)))
unit_flags = $($(word 3,$(subst =, ,$(1))))
define NL


endef

LIB_SRCS := $(foreach u,$(UNITS),$(call unit_src,$(u)))
LIB_HDRS := $(wildcard $(CSRC)/*.h) include/vame.h
OBJDIR   := $(PKG)/build
# $(call build_lib,<output .so>,<extra flags>): every unit with its own flags, then one link
define build_lib
	@mkdir -p $(LIBDIR) $(OBJDIR)
	$(foreach u,$(UNITS),$(HIPCC) $(HIPFLAGS) $(call unit_flags,$(u)) $(2) -c -o $(OBJDIR)/$(notdir $(1)).$(call unit_tag,$(u)).o $(call unit_src,$(u))$(NL))
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared -o $(1) $(foreach u,$(UNITS),$(OBJDIR)/$(notdir $(1)).$(call unit_tag,$(u)).o)
endef

all: lib cli synth oracle probe

lib: $(LIBDIR)/libvame.so

# synthetic test-sequence generator (bench / tests only; vame/synth.py is its spec)
synth: $(LIBDIR)/libvame_synth.so
$(LIBDIR)/libvame_synth.so: $(CSRC)/vame_synth.c
	@mkdir -p $(LIBDIR)
	gcc -O2 -fopenmp -ffp-contract=off -fPIC -shared -Wall -o $@ $<

# timing-only ablation builds (results are wrong): make ablate [ABLATE_SET="..."]
ABLATE_SET ?= 1 2 4 6 7 8 11 13 14 15 16 32
ablate:
	@mkdir -p $(LIBDIR)
	for a in $(ABLATE_SET); do $(MAKE) -s variant NAME=ablate$$a DEFS=-DVAME_ABLATE=$$a || exit 1; done
# experiment builds: make variant NAME=x DEFS="-DFOO=1" -> lib/libvame_x.so
variant:
	$(call build_lib,$(LIBDIR)/libvame_$(NAME).so,$(DEFS))
# instrumentation build counting the sub-block predictions run: make count
count:
	$(call build_lib,$(LIBDIR)/libvame_count.so,-DVAME_COUNT_PRED=1)
# profiling-only build with per-phase shader-clock counters: make phase
phase:
	$(call build_lib,$(LIBDIR)/libvame_phase.so,-DVAME_PHASE_TIMING=1)

cli: $(BINDIR)/vame

# does an event after a call wait for its any-order kernels? (tests/test_gpu_parity.py)
probe: tests/native/anyorder_probe
tests/native/anyorder_probe: tests/native/anyorder_probe.hip
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -Wall -o $@ $<

$(LIBDIR)/libvame.so: $(LIB_SRCS) $(LIB_HDRS)
	$(call build_lib,$@,)

# cli_options / cli_plan are host-only (no HIP include; tests/native/cli_check.cpp
# builds them with g++), cli_worker and vame_main call HIP
CLI_SRCS := $(addprefix $(PKG)/host/,vame_main.cpp cli_worker.cpp cli_options.cpp cli_plan.cpp)
CLI_HDRS := $(wildcard $(PKG)/host/*.h) include/vame.h
$(BINDIR)/vame: $(CLI_SRCS) $(CLI_HDRS) $(LIBDIR)/libvame.so
	@mkdir -p $(BINDIR)
	$(HIPCC) -O2 -std=c++17 -Wall -o $@ $(CLI_SRCS) \
	    -L$(LIBDIR) -lvame -Wl,-rpath,'$$ORIGIN/../lib' -lpthread

oracle:
	$(MAKE) -s -C oracle libvame_oracle.so
	@if [ -d /root/reference ]; then $(MAKE) -s -C oracle ref; fi

resource-usage:
	$(foreach u,$(UNITS),$(if $(filter %.hip,$(call unit_src,$(u))),$(HIPCC) $(HIPFLAGS) $(call unit_flags,$(u)) -Rpass-analysis=kernel-resource-usage -c -o /dev/null $(call unit_src,$(u))$(NL)))

clean:
	rm -rf $(LIBDIR) $(BINDIR) $(OBJDIR)
	$(MAKE) -s -C oracle clean

.PHONY: all lib cli synth oracle probe clean resource-usage ablate phase variant count
