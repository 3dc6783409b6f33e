# tests/emul/pathseq.mk -- TEST-ONLY: the path-sequence program of graphaligner_amd/csrc/ga_pathseq.h compiled for the host, with its
# component hook (ga_emul_pathseq.cpp).  Output tests/_build/libga_pathseq_emul.so, a library of its own next to the back end's emulation.
# Never shipped, never loaded by graphaligner_amd/.
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
SRC := $(HERE)../../graphaligner_amd/csrc
OUT := $(HERE)../_build
CXXFLAGS := -std=c++17 -O2 -g -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter -Wno-unknown-pragmas
EMUL := -DGA_EMULATE=1 -DGA_WAVE_HEADER='"$(HERE)ga_wave_emul.h"'

$(OUT)/libga_pathseq_emul.so: $(HERE)ga_emul_pathseq.cpp $(wildcard $(SRC)/*.h)
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) $(EMUL) -shared -o $@ $<

# the stand-alone check of the same code under the sanitizers (pathseq_stream_check.cpp): make -f pathseq.mk check
# builds it and runs it over the file tests/pathseq_stream_dump.py writes
SANITIZE := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer

$(OUT)/pathseq_stream_check: $(HERE)pathseq_stream_check.cpp $(HERE)ga_emul_pathseq.cpp $(wildcard $(SRC)/*.h)
	@mkdir -p $(OUT)
	$(CXX) $(filter-out -fPIC,$(CXXFLAGS)) -O1 $(SANITIZE) $(EMUL) -o $@ $<

check: $(OUT)/pathseq_stream_check
	python3 $(HERE)../pathseq_stream_dump.py $(OUT)/pathseq_streams.txt
	$(OUT)/pathseq_stream_check $(OUT)/pathseq_streams.txt

.PHONY: check
