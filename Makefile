# Builds everything in-tree:
#   yadcc_amd/libydc.so        HIP kernels + C-ABI (+ host C++ dispatcher), gfx950
#   oracle/liboracle.so, oracle/_ref/libyadcc_ref.so   (test infrastructure)
#   tests/model/libmodel.so    (test tool)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := yadcc_amd/csrc
HIP_SRCS := $(CSRC)/ydc_api.hip $(wildcard $(CSRC)/*.cc)
HDRS := $(wildcard $(CSRC)/*.h) include/yadcc_dispatch.h

all: lib oracle model native

lib: yadcc_amd/libydc.so
yadcc_amd/libydc.so: $(HIP_SRCS) $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -shared -Wall -Wno-unused-function \
	    -Iinclude -I$(CSRC) -o $@ $(HIP_SRCS)

# Measurement build: the matching kernel leaves phase stamps behind (tools/phase_probe.py).
probe: yadcc_amd/libydc_probe.so
yadcc_amd/libydc_probe.so: $(HIP_SRCS) $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -shared -Wall -Wno-unused-function \
	    -DYDC_PHASE_PROBE -Iinclude -I$(CSRC) -o $@ $(HIP_SRCS)

oracle:
	$(MAKE) -s -C oracle
model:
	$(MAKE) -s -C tests/model
# Native (C++) drive of the dispatcher through the scheduler harness; plain g++, links libydc.so.
native: tests/native/harness_test tests/native/td_linearize_gpu tools/td_native_bench tools/hbm_calib tests/tools/launch_probe tests/tools/overlap_probe tests/tools/atomic_probe tests/native/key_forms_gpu
	$(MAKE) -s -C tests/native all
# Counter calibration microbenchmark (tools/calibrate.sh runs it under rocprofv3 on the GPU box).
tools/hbm_calib: tools/hbm_calib.hip
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o $@ tools/hbm_calib.hip
# Launch latency / resident mailbox and two-queue overlap microbenchmarks.
tests/tools/launch_probe: tests/tools/launch_probe.hip
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o $@ tests/tools/launch_probe.hip
tests/tools/overlap_probe: tests/tools/overlap_probe.hip
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o $@ tests/tools/overlap_probe.hip
tests/tools/atomic_probe: tests/tools/atomic_probe.hip
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o $@ tests/tools/atomic_probe.hip
# The closed forms of dispatch_core.h, one thread per case (tests/test_key_forms_gpu.py).
tests/native/key_forms_gpu: tests/native/key_forms_gpu.hip tests/native/key_forms.h $(CSRC)/dispatch_core.h
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -Wall -o $@ tests/native/key_forms_gpu.hip
tools/td_native_bench: tools/td_native_bench.cc tools/parked_workload.h yadcc_amd/libydc.so $(HDRS)
	g++ -O2 -std=c++17 -Wall -I$(CSRC) -Iinclude -Itools -o $@ tools/td_native_bench.cc \
	    -Lyadcc_amd -lydc -Wl,-rpath,'$$ORIGIN/../yadcc_amd' -lpthread
# The same tool over the CPU stand-in of the device API (host-side profiling without a GPU).
tools/td_native_bench_stub: tools/td_native_bench.cc tools/parked_workload.h $(HDRS)
	$(MAKE) -s -C tests/native all
	g++ -O2 -g -std=c++17 -Wall -I$(CSRC) -Iinclude -Itools -o $@ tools/td_native_bench.cc \
	    -Ltests/native -ltd_stub -Wl,-rpath,'$$ORIGIN/../tests/native' -lpthread
tests/native/harness_test: tests/native/harness_test.cc tests/native/scheduler_harness.cc tests/native/scheduler_harness.h yadcc_amd/libydc.so $(HDRS)
	g++ -O2 -std=c++17 -Wall -I$(CSRC) -Iinclude -Itests/native -o $@ tests/native/harness_test.cc tests/native/scheduler_harness.cc \
	    -Lyadcc_amd -lydc -Wl,-rpath,'$$ORIGIN/../../yadcc_amd' -lpthread
# Concurrent callers through the C-ABI against the real library (verified against the reference by
# tests/test_task_dispatcher_gpu.py).
tests/native/td_linearize_gpu: tests/native/td_linearize.cc yadcc_amd/libydc.so include/yadcc_dispatch.h
	g++ -O2 -std=c++17 -Wall -Iinclude -o $@ tests/native/td_linearize.cc \
	    -Lyadcc_amd -lydc -Wl,-rpath,'$$ORIGIN/../../yadcc_amd' -lpthread
# Sanitizer builds of the host class against the CPU stand-in of the device API, and of the
# headers that are free of HIP (no GPU).
tsan asan flatmap shardplan:
	$(MAKE) -s -C tests/native $@
# The lane-choice rule of the pipelined batches (lane_rule.h) row by row, ASan + UBSan, no GPU
# (tests/test_lane_rule.py builds and runs the same program).
tests/native/lane_rule_test: tests/native/lane_rule_test.cc $(CSRC)/lane_rule.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) -o $@ tests/native/lane_rule_test.cc
lanerule: tests/native/lane_rule_test
	tests/native/lane_rule_test
# The occupancy rule of a batch (occupancy_plan.h: the bin sort's width) against a written table,
# ASan + UBSan, no GPU (tests/test_occupancy_plan.py builds and runs the same program).
tests/native/occupancy_plan_test: tests/native/occupancy_plan_test.cc $(CSRC)/occupancy_plan.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) -o $@ tests/native/occupancy_plan_test.cc
occupancyplan: tests/native/occupancy_plan_test
	tests/native/occupancy_plan_test
# The admission arithmetic (admit_clip.h) against its written rule with 128-bit sums, ASan + UBSan, no GPU
# (tests/test_stream_requestor_model.py builds and runs the same program).
tests/native/admit_clip_test: tests/native/admit_clip_test.cc $(CSRC)/admit_clip.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) -o $@ tests/native/admit_clip_test.cc
admitclip: tests/native/admit_clip_test
	tests/native/admit_clip_test
# The predicate of the lease select (lease_filter.h) against a second restatement, all 2^9 combinations of
# its predicates on edge values, ASan + UBSan, no GPU (tests/test_stream_select_binding.py builds and runs
# the same program).
tests/native/lease_filter_test: tests/native/lease_filter_test.cc $(CSRC)/lease_filter.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) -o $@ tests/native/lease_filter_test.cc
leasefilter: tests/native/lease_filter_test
	tests/native/lease_filter_test
# The fair-share arithmetic (fair_level.h) against the literal progressive fill with 128-bit sums, ASan + UBSan,
# no GPU (tests/test_stream_fair_binding.py builds and runs the same program).
tests/native/fair_level_test: tests/native/fair_level_test.cc $(CSRC)/fair_level.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) -o $@ tests/native/fair_level_test.cc
fairlevel: tests/native/fair_level_test
	tests/native/fair_level_test
# The interval arithmetic of the usage accounting (usage_quanta.h) against its rule with 128-bit intermediates,
# ASan + UBSan, no GPU (tests/test_stream_usage_binding.py builds and runs the same program).
tests/native/usage_quanta_test: tests/native/usage_quanta_test.cc $(CSRC)/usage_quanta.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) -o $@ tests/native/usage_quanta_test.cc
usagequanta: tests/native/usage_quanta_test
	tests/native/usage_quanta_test
# The home slot and the slot counts of the three hashed tables (index_home.h), printed for the restatement of
# tests/hash_index_cases.py, ASan + UBSan, no GPU (tests/test_hash_index_model.py and tests/test_usage_table_model.py
# build and run the same program).
tests/native/hash_home_test: tests/native/hash_home_test.cc $(CSRC)/index_home.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) -o $@ tests/native/hash_home_test.cc
hashhome: tests/native/hash_home_test
	printf 'k 0\nk 9e3779b97f4a7c15\ns 512\ns 513\nu 512\nu 513\n' | tests/native/hash_home_test
clean:
	rm -f yadcc_amd/libydc.so tests/model/libmodel.so tests/native/lane_rule_test tests/native/admit_clip_test tests/native/occupancy_plan_test tests/native/lease_filter_test tests/native/fair_level_test tests/native/hash_home_test tests/native/usage_quanta_test
	$(MAKE) -C tests/native clean
	$(MAKE) -C oracle clean
.PHONY: all lib probe oracle model native tsan asan flatmap shardplan admitclip lanerule occupancyplan leasefilter fairlevel usagequanta hashhome clean
