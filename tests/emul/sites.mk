# tests/emul/sites.mk -- TEST-ONLY: the site-query program of graphaligner_amd/csrc/ga_sites.h compiled for the host, with its component
# hook and a stub back end (ga_emul_sites.cpp) behind the product's host code.  Output tests/_build/libga_sites_emul.so, a library of
# its own next to the back end's emulation.  Never shipped, never loaded by graphaligner_amd/.
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
SRC := $(HERE)../../graphaligner_amd/csrc
OUT := $(HERE)../_build
CXXFLAGS := -std=c++17 -O2 -g -fPIC -ffp-contract=off -Wall -Wextra -Wno-unused-parameter -Wno-unknown-pragmas
EMUL := -DGA_EMULATE=1 -DGA_WAVE_HEADER='"$(HERE)ga_wave_emul.h"'
HOST := $(SRC)/ga_host.cpp $(SRC)/ga_vgio.cpp $(SRC)/ga_seed_host.cpp

$(OUT)/libga_sites_emul.so: $(HERE)ga_emul_sites.cpp $(HOST) $(wildcard $(SRC)/*.h) $(HERE)../../include/graphaligner_amd.h
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) $(EMUL) -shared -pthread -o $@ $< $(HOST) -lz

# the stand-alone check of the same code under the sanitizers (sites_check.cpp, a main of its own): make -f sites.mk check
SANITIZE := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer

$(OUT)/sites_check: $(HERE)sites_check.cpp $(HERE)ga_emul_sites.cpp $(HOST) $(wildcard $(SRC)/*.h)
	@mkdir -p $(OUT)
	$(CXX) $(filter-out -fPIC,$(CXXFLAGS)) -O1 $(SANITIZE) $(EMUL) -pthread -o $@ $< $(HOST) -lz

check: $(OUT)/sites_check
	$(OUT)/sites_check

.PHONY: check
