# Build recipe for the MI355X-native alignment engine.
#   make lib     -> vg_amd/libvgamd.so        HIP kernels + C ABI (gfx950)
#   make host    -> vg_amd/libvgamd_host.so   C++ host shim mirroring vg's Aligner interface
#   make oracle  -> oracle/libvgoracle.so     CPU oracle (test infrastructure only)
# Built artefacts are git-ignored; they travel to the GPU box with gpurun.

HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++
CC       ?= gcc
ARCH     ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Iinclude -Wall -Wno-unused-function -Wno-unused-value
CXXFLAGS ?= -O2 -std=c++17 -fPIC -Iinclude -Wall
CFLAGS   ?= -O3 -march=x86-64-v2 -std=c11 -fPIC -fopenmp -Iinclude -Wall

LIB_SRCS    := $(wildcard vg_amd/csrc/*.hip) $(wildcard vg_amd/csrc/*.cpp)
LIB_HDRS    := $(wildcard vg_amd/csrc/*.h vg_amd/csrc/*.hpp include/*.h)
HOST_SRCS   := $(wildcard vg_amd/host/*.cpp) $(wildcard vg_amd/host/vg_standin/*.cpp)
HOST_HDRS   := $(wildcard vg_amd/host/*.hpp vg_amd/host/vg_standin/*.hpp include/*.h)
ORACLE_SRCS := $(wildcard oracle/*.c)

all: lib host oracle
lib: vg_amd/libvgamd.so
host: vg_amd/libvgamd_host.so
oracle: oracle/libvgoracle.so

# the C-ABI/packing layer is plain C++; only the .hip files carry device code
LIB_CPP_OBJS := $(patsubst %.cpp,%.o,$(wildcard vg_amd/csrc/*.cpp))
LIB_HIP_OBJS := $(patsubst %.hip,%.o,$(wildcard vg_amd/csrc/*.hip))
vg_amd/csrc/%.o: vg_amd/csrc/%.cpp $(LIB_HDRS)
	$(CXX) $(CXXFLAGS) -O3 -c $< -o $@
vg_amd/csrc/%.o: vg_amd/csrc/%.hip $(LIB_HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
vg_amd/libvgamd.so: $(LIB_CPP_OBJS) $(LIB_HIP_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(LIB_CPP_OBJS) $(LIB_HIP_OBJS)

vg_amd/libvgamd_host.so: $(HOST_SRCS) $(HOST_HDRS)
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOST_SRCS) -ldl

oracle/libvgoracle.so: $(ORACLE_SRCS) include/vgk.h oracle/vgo_haplo.h
	$(CC) $(CFLAGS) -shared -o $@ $(ORACLE_SRCS)

clean:
	rm -f vg_amd/csrc/*.o vg_amd/libvgamd.so vg_amd/libvgamd_host.so oracle/libvgoracle.so

.PHONY: all lib host oracle clean

# test-only: CPU lock-step emulation of the HIP lane code behind the same C ABI (VGK_PK_CHECK: pk16.hpp's full-width adds and subtracts count
# every call that carries or borrows across the halves)
emu: tests/emu/libvgamd_emu.so
EMU_OBJS := $(patsubst vg_amd/csrc/%.cpp,tests/emu/obj/%.o,$(wildcard vg_amd/csrc/*.cpp)) tests/emu/obj/backend_emu.o
tests/emu/obj/%.o: vg_amd/csrc/%.cpp $(LIB_HDRS)
	@mkdir -p tests/emu/obj
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -DVGK_PK_CHECK -c $< -o $@
tests/emu/obj/backend_emu.o: tests/emu/backend_emu.cpp $(LIB_HDRS)
	@mkdir -p tests/emu/obj
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -DVGK_PK_CHECK -c $< -o $@
tests/emu/libvgamd_emu.so: $(EMU_OBJS)
	$(CXX) -shared -o $@ $(EMU_OBJS) -lpthread
.PHONY: emu

# test-only: the serial form of find_seeds' choice on the device (minimizer_device.hpp: mz_choose_one) behind one C call
choose: tests/emu/libvgamd_choose.so
tests/emu/libvgamd_choose.so: tests/emu/choose_driver.cpp $(LIB_HDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -Wno-unknown-pragmas -shared -o $@ $<
.PHONY: choose

# test-only: the serial form of the chaining rule on the device (chain_items_device.hpp: ci_problem_one) behind one C call
chainitems: tests/emu/libvgamd_chainitems.so
tests/emu/libvgamd_chainitems.so: tests/emu/chain_items_driver.cpp $(LIB_HDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -Wno-unknown-pragmas -shared -o $@ $<
.PHONY: chainitems

# test-only: the serial form of the device rule that packs windows of a resident graph for the wide kernels (gssw_wide_pack_device.hpp) beside the
# host packer of explicit graphs (gssw_wide_pack.hpp) behind one C call
widewin: tests/emu/libvgamd_widewin.so
tests/emu/libvgamd_widewin.so: tests/emu/wide_windows_driver.cpp $(LIB_HDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -Wno-unknown-pragmas -shared -o $@ $<
.PHONY: widewin

# test-only: the serial form of the device rule that makes chaining anchors from seeds and gapless extensions (extension_anchors_device.hpp:
# ea_problem_one) behind one C call, and the same as a program of its own under the host sanitizers
extanchors: tests/emu/libvgamd_extanchors.so
tests/emu/libvgamd_extanchors.so: tests/emu/extension_anchors_driver.cpp $(LIB_HDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -Wno-unknown-pragmas -shared -o $@ $<
extanchors_san: tests/emu/extension_anchors_san
tests/emu/extension_anchors_san: tests/emu/extension_anchors_driver.cpp $(LIB_HDRS)
	$(CXX) -O1 -g -std=c++17 -Iinclude -Wall -Wno-unknown-pragmas -DEA_DRIVER_MAIN -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
.PHONY: extanchors extanchors_san

# test-only: the serial form of the device rule that composes a short read's alignments from its extension set and its tails
# (read_alignments_device.hpp: ra_read_one) behind one C call, and the same as a program of its own under the host sanitizers
readaln: tests/emu/libvgamd_readaln.so
tests/emu/libvgamd_readaln.so: tests/emu/read_alignments_driver.cpp $(LIB_HDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -Wno-unknown-pragmas -shared -o $@ $<
readaln_san: tests/emu/read_alignments_san
tests/emu/read_alignments_san: tests/emu/read_alignments_driver.cpp $(LIB_HDRS)
	$(CXX) -O1 -g -std=c++17 -Iinclude -Wall -Wno-unknown-pragmas -DRA_DRIVER_MAIN -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
.PHONY: readaln readaln_san

# test-only: the serial form of the device rules for a read's mapping quality — agglomerations, the scores' quality and the explored cap
# (read_mapq_device.hpp: mq_region_one, mq_read_one) behind one C call each, and the same as a program of its own under the host sanitizers
readmapq: tests/emu/libvgamd_readmapq.so
tests/emu/libvgamd_readmapq.so: tests/emu/read_mapq_driver.cpp $(LIB_HDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -Wno-unknown-pragmas -ffp-contract=off -shared -o $@ $<
readmapq_san: tests/emu/read_mapq_san
tests/emu/read_mapq_san: tests/emu/read_mapq_driver.cpp $(LIB_HDRS)
	$(CXX) -O1 -g -std=c++17 -Iinclude -Wall -Wno-unknown-pragmas -ffp-contract=off -DMQ_DRIVER_MAIN -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
.PHONY: readmapq readmapq_san

# test-only: the serial form of the device rules for a short read's funnel — cluster scores, the three walks, the write-out (read_funnel_device.hpp:
# rf_walk and the rf_*_one around it) behind one C call each, and the same as a program of its own under the host sanitizers
readfunnel: tests/emu/libvgamd_readfunnel.so
tests/emu/libvgamd_readfunnel.so: tests/emu/read_funnel_driver.cpp $(LIB_HDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -Wno-unknown-pragmas -ffp-contract=off -shared -o $@ $<
readfunnel_san: tests/emu/read_funnel_san
tests/emu/read_funnel_san: tests/emu/read_funnel_driver.cpp $(LIB_HDRS)
	$(CXX) -O1 -g -std=c++17 -Iinclude -Wall -Wno-unknown-pragmas -ffp-contract=off -DFN_DRIVER_MAIN -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
.PHONY: readfunnel readfunnel_san

# test-only: the serial composition of the device rule for a chain's links — the checks, the walk, the counts and the write-out
# (chain_links_device.hpp: cl_check_one, cl_walk_one, cl_count_one, cl_write_one) behind one C call, and the same as a program of its own under the
# host sanitizers
chainlinks: tests/emu/libvgamd_chainlinks.so
tests/emu/libvgamd_chainlinks.so: tests/emu/chain_links_driver.cpp $(LIB_HDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -Wno-unknown-pragmas -shared -o $@ $<
chainlinks_san: tests/emu/chain_links_san
tests/emu/chain_links_san: tests/emu/chain_links_driver.cpp $(LIB_HDRS)
	$(CXX) -O1 -g -std=c++17 -Iinclude -Wall -Wno-unknown-pragmas -DCL_DRIVER_MAIN -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
.PHONY: chainlinks chainlinks_san

# test-only: the serial composition of the device rule for a long read's mappings — the checks, the statistics, multiplicities and sort scores, the pick
# on one lane (pick_mappings_device.hpp: pick_check_one, pick_stat_one, pick_alignment_one, pick_read_one) behind one C call, and the same as a program of
# its own under the host sanitizers
pickmappings: tests/emu/libvgamd_pickmappings.so
tests/emu/libvgamd_pickmappings.so: tests/emu/pick_mappings_driver.cpp $(LIB_HDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -Wno-unknown-pragmas -ffp-contract=off -shared -o $@ $<
pickmappings_san: tests/emu/pick_mappings_san
tests/emu/pick_mappings_san: tests/emu/pick_mappings_driver.cpp $(LIB_HDRS)
	$(CXX) -O1 -g -std=c++17 -Iinclude -Wall -Wno-unknown-pragmas -ffp-contract=off -DPICK_DRIVER_MAIN -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
.PHONY: pickmappings pickmappings_san

# test-only: the serial form of the device rule for a pair's mapping qualities — pair scores, their order, the shared caps (pair_mapq_device.hpp:
# pm_candidate_score, pm_pair_one; the mates' caps by read_mapq_device.hpp's mq_cap_one) behind one C call, and the same as a program of its own under
# the host sanitizers
pairmapq: tests/emu/libvgamd_pairmapq.so
tests/emu/libvgamd_pairmapq.so: tests/emu/pair_mapq_driver.cpp $(LIB_HDRS)
	$(CXX) -O2 -g -std=c++17 -fPIC -Iinclude -Wall -Wno-unknown-pragmas -ffp-contract=off -shared -o $@ $<
pairmapq_san: tests/emu/pair_mapq_san
tests/emu/pair_mapq_san: tests/emu/pair_mapq_driver.cpp $(LIB_HDRS)
	$(CXX) -O1 -g -std=c++17 -Iinclude -Wall -Wno-unknown-pragmas -ffp-contract=off -DPM_DRIVER_MAIN -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
.PHONY: pairmapq pairmapq_san

# test-only: vgk_haplo_create + vgk_gapless_extend on the emulated backend as a program of its own under the host sanitizers — the lane code of
# gapless_device.hpp and its per-thread slabs on the limits the edge corpus of tests/test_gapless_definition.py sits on
gapless_san: tests/emu/gapless_san
SAN_FLAGS := -O1 -g -std=c++17 -Iinclude -Wall -DVGK_PK_CHECK -fsanitize=address,undefined -fno-sanitize-recover=undefined
SAN_ENGINE_OBJS := $(patsubst vg_amd/csrc/%.cpp,tests/emu/san_obj/%.o,$(wildcard vg_amd/csrc/*.cpp)) tests/emu/san_obj/backend_emu.o
SAN_OBJS := $(SAN_ENGINE_OBJS) tests/emu/san_obj/gapless_san_main.o
tests/emu/san_obj/%.o: vg_amd/csrc/%.cpp $(LIB_HDRS)
	@mkdir -p tests/emu/san_obj
	$(CXX) $(SAN_FLAGS) -c $< -o $@
tests/emu/san_obj/%.o: tests/emu/%.cpp $(LIB_HDRS)
	@mkdir -p tests/emu/san_obj
	$(CXX) $(SAN_FLAGS) -c $< -o $@
tests/emu/gapless_san: $(SAN_OBJS)
	$(CXX) -fsanitize=address,undefined -o $@ $(SAN_OBJS) -lpthread
.PHONY: gapless_san

# test-only: vgk_haplo_create + vgk_chain_stitch on the emulated backend as a program of its own under the host sanitizers (the same sanitized
# engine objects, its own main) — the lane code of chain_device.hpp on the calls of tests/test_chain_stitch_definition.py
chainstitch_san: tests/emu/chain_stitch_san
CHAINSTITCH_SAN_OBJS := $(SAN_ENGINE_OBJS) tests/emu/san_obj/chain_stitch_san_main.o
tests/emu/chain_stitch_san: $(CHAINSTITCH_SAN_OBJS)
	$(CXX) -fsanitize=address,undefined -o $@ $(CHAINSTITCH_SAN_OBJS) -lpthread
.PHONY: chainstitch_san

# test-only: the launch plans of launch_split.hpp (which item in which launch, which slice of the slab) against a brute force, as a program of its
# own under the host sanitizers — the header alone, no engine object
launch_split_san: tests/emu/launch_split_san
tests/emu/launch_split_san: tests/emu/launch_split_san_main.cpp vg_amd/csrc/launch_split.hpp include/vgk.h
	$(CXX) $(SAN_FLAGS) -Ivg_amd/csrc -o $@ $<
.PHONY: launch_split_san
