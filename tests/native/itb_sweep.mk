# tests/native/itb_sweep.mk -- CPU harnesses of the ITB sweep
# (pomegranate_amd/csrc/itb_sweep.h as plain C++; never part of the product
# library).
# Built by __graft_entry__.build(): make -f itb_sweep.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
INCLUDE := $(abspath $(HERE)../../include)
CXXFLAGS_SWEEP = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(INCLUDE)
# itb_sweep_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
SWEEP_DEPS = $(HERE)itb_sweep_host.cc $(CSRC)/itb_sweep.h $(CSRC)/itb_split.h $(CSRC)/itb_check.h $(CSRC)/itb_find.h \
    $(CSRC)/itb_scan.h $(INCLUDE)/pom_sweep.h $(INCLUDE)/pom_split.h $(INCLUDE)/pom_check.h $(INCLUDE)/pom_lookup.h \
    $(INCLUDE)/pom_readdir.h $(INCLUDE)/pom_gc.h

all: $(HERE)libitb_sweep_host.so $(HERE)itb_sweep_check

$(HERE)libitb_sweep_host.so: $(SWEEP_DEPS)
	$(CXX) $(CXXFLAGS_SWEEP) -fPIC -shared -o $@ $<

$(HERE)itb_sweep_check: $(SWEEP_DEPS)
	$(CXX) $(CXXFLAGS_SWEEP) $(SAN) -DITB_SWEEP_CHECK -o $@ $<

clean:
	rm -f $(HERE)libitb_sweep_host.so $(HERE)itb_sweep_check

.PHONY: all clean
