# tests/emul/edges.mk -- TEST-ONLY: the edge-support program of graphaligner_amd/csrc/ga_edges.h compiled for the host, with its component
# hook (ga_emul_edges.cpp).  Output tests/_build/libga_edges_emul.so, a library of its own next to the back end's emulation.
# Never shipped, never loaded by graphaligner_amd/.
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
SRC := $(HERE)../../graphaligner_amd/csrc
OUT := $(HERE)../_build
CXXFLAGS := -std=c++17 -O2 -g -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter -Wno-unknown-pragmas
EMUL := -DGA_EMULATE=1 -DGA_WAVE_HEADER='"$(HERE)ga_wave_emul.h"'

$(OUT)/libga_edges_emul.so: $(HERE)ga_emul_edges.cpp $(wildcard $(SRC)/*.h)
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) $(EMUL) -shared -o $@ $<

# the stand-alone check of the same code under the sanitizers (edges_stream_check.cpp): make -f edges.mk check
# builds it and runs it over the file tests/edge_stream_dump.py writes.  The host library's sources are compiled in, with no back end
HOST := $(SRC)/ga_host.cpp $(SRC)/ga_vgio.cpp $(SRC)/ga_seed_host.cpp
SANITIZE := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer

$(OUT)/edges_stream_check: $(HERE)edges_stream_check.cpp $(HERE)ga_emul_edges.cpp $(HOST) $(wildcard $(SRC)/*.h)
	@mkdir -p $(OUT)
	$(CXX) $(filter-out -fPIC,$(CXXFLAGS)) -O1 $(SANITIZE) $(EMUL) -pthread -o $@ $< $(HOST) -lz

check: $(OUT)/edges_stream_check
	python3 $(HERE)../edge_stream_dump.py $(OUT)/edge_streams.txt
	$(OUT)/edges_stream_check $(OUT)/edge_streams.txt

.PHONY: check
