# Makefile -- the same builds __graft_entry__.build() drives from Python, for C++ integrators.
#   make lib         beamforming-lk_amd/libawpu_hip.so   (hipcc, gfx950 only; there is no CPU fallback)
#   make oracle      oracle/liboracle_das.so (+ oracle/_ref from the reference tree when it is present)
#   make example     examples/heatmap_min: the C ABI from plain C (needs an MI355X to do more than report its absence)
#   make host-test   tests/host/test_mimo_worker: the C++ mirror (MIMOWorkerHip, AWProcessingUnitHip,
#                    PipelineHip) against the oracle; needs an MI355X to run (--nogpu checks the failure path);
#                    tests/host/test_exact_signatures: class AWProcessingUnit with the reference's own signatures
#                    (-DAWPU_WITH_OPENCV; cv::Mat from OPENCV_CFLAGS)
HIPCC ?= /opt/rocm/bin/hipcc
PKG := beamforming-lk_amd
CSRC := $(PKG)/csrc
LIB := $(PKG)/libawpu_hip.so
KERNEL_SRC := $(CSRC)/das_kernels.hip $(CSRC)/das_fast.hip $(CSRC)/track_kernels.hip $(CSRC)/block_kernels.hip $(CSRC)/watch_kernels.hip $(CSRC)/find_kernels.hip $(CSRC)/band_kernels.hip $(CSRC)/spectral_kernels.hip $(CSRC)/expose_kernels.hip $(CSRC)/cohere_kernels.hip $(CSRC)/peel_kernels.hip $(CSRC)/awpu_hip.cpp \
              $(CSRC)/awpu_group.cpp $(CSRC)/awpu_sweep.cpp $(CSRC)/awpu_runs.cpp $(CSRC)/geometry_host.cpp $(CSRC)/find_host.cpp $(CSRC)/band_host.cpp $(CSRC)/spectral_host.cpp $(CSRC)/awpu_focus.cpp $(CSRC)/expose_host.cpp $(CSRC)/awpu_cohere.cpp $(CSRC)/cohere_host.cpp $(CSRC)/awpu_peel.cpp $(CSRC)/peel_host.cpp
HOST_SRC := $(PKG)/host/mimo_worker_hip.cpp $(PKG)/host/aw_processing_unit_hip.cpp $(PKG)/host/pipeline_hip.cpp \
            $(PKG)/host/aw_processing_unit.cpp $(PKG)/host/spherical_gradient_hip.cpp
# OPENCV_CFLAGS: where <opencv2/core.hpp> lives; defaults to the tests' few-line stand-in for cv::Mat (no OpenCV here)
OPENCV_CFLAGS ?= -Itests/host/mock_opencv

.PHONY: lib oracle host-test example trips clean
lib: $(LIB)

$(LIB): $(KERNEL_SRC) $(CSRC)/awpu_handle.h $(CSRC)/das_kernels.h $(CSRC)/sweep_plan.h $(CSRC)/nd_tile_window.h $(CSRC)/block_kernels.h $(CSRC)/watch_kernels.h $(CSRC)/find_kernels.h $(CSRC)/find_rule.h $(CSRC)/band_kernels.h $(CSRC)/band_rule.h $(CSRC)/spectral_kernels.h $(CSRC)/spectral_rule.h $(CSRC)/expose_kernels.h $(CSRC)/expose_rule.h $(CSRC)/cohere_kernels.h $(CSRC)/cohere_rule.h $(CSRC)/peel_kernels.h $(CSRC)/peel_rule.h $(CSRC)/das_fast_trip.inc include/awpu_hip.h include/awpu_hip_track.h \
        include/awpu_hip_blocks.h include/awpu_hip_listen.h include/awpu_hip_watch.h include/awpu_hip_find.h include/awpu_hip_band.h include/awpu_hip_spectral.h include/awpu_hip_expose.h include/awpu_hip_cohere.h include/awpu_hip_peel.h
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -Wno-unused-result -Werror=inline-asm -x hip \
	    -Iinclude -I$(CSRC) $(KERNEL_SRC) -o $@

# the hand-scheduled inner loops are GENERATED at build time (tools/gen_trip_asm.py documents the schedule and its knobs;
# the include is not tracked)
$(CSRC)/das_fast_trip.inc: tools/gen_trip_asm.py
	python3 tools/gen_trip_asm.py

trips: $(CSRC)/das_fast_trip.inc

oracle:
	$(MAKE) -C oracle

host-test: $(LIB) oracle
	g++ -O2 -std=c++17 -pthread -Iinclude -I$(PKG)/host -Ioracle tests/host/test_mimo_worker.cpp $(HOST_SRC) \
	    -L$(PKG) -lawpu_hip -Loracle -loracle_das -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -Wl,-rpath,'$$ORIGIN/../../oracle' -Wl,-rpath,/opt/rocm/lib \
	    -o tests/host/test_mimo_worker
	g++ -O2 -std=c++17 -pthread -DAWPU_WITH_OPENCV $(OPENCV_CFLAGS) -Iinclude -I$(PKG)/host -Ioracle tests/host/test_exact_signatures.cpp $(HOST_SRC) \
	    -L$(PKG) -lawpu_hip -Loracle -loracle_das -Wl,-rpath,'$$ORIGIN/../../$(PKG)' -Wl,-rpath,'$$ORIGIN/../../oracle' -Wl,-rpath,/opt/rocm/lib \
	    -o tests/host/test_exact_signatures
	g++ -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -I$(PKG)/host tests/host/test_spherical_gradient.cpp \
	    $(PKG)/host/spherical_gradient_hip.cpp -L$(PKG) -lawpu_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../$(PKG)' \
	    -Wl,-rpath,/opt/rocm/lib -o tests/host/test_spherical_gradient

example: $(LIB)
	gcc -O2 -Wall -Iinclude examples/heatmap_min.c -L$(PKG) -lawpu_hip -lm -Wl,-rpath,'$$ORIGIN/../$(PKG)' \
	    -Wl,-rpath,/opt/rocm/lib -o examples/heatmap_min
	gcc -O2 -Wall -Iinclude examples/live_call_rate.c -L$(PKG) -lawpu_hip -lm -Wl,-rpath,'$$ORIGIN/../$(PKG)' \
	    -Wl,-rpath,/opt/rocm/lib -o examples/live_call_rate

clean:
	rm -f $(LIB) tests/host/test_mimo_worker tests/host/test_exact_signatures tests/host/test_spherical_gradient examples/heatmap_min examples/live_call_rate
	$(MAKE) -C oracle clean
