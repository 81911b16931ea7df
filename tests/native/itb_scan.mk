# tests/native/itb_scan.mk -- CPU harnesses of the garbage collector's ITB walk
# (pomegranate_amd/csrc/itb_scan.h as plain C++; never part of the product
# library).  Built by __graft_entry__.build(): make -f itb_scan.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
CXXFLAGS_SCAN = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(abspath $(HERE)../../include)
# itb_scan_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
SCAN_DEPS = $(HERE)itb_scan_host.cc $(CSRC)/itb_scan.h $(HERE)../../include/pom_gc.h

all: $(HERE)libitb_scan_host.so $(HERE)itb_scan_check

$(HERE)libitb_scan_host.so: $(SCAN_DEPS)
	$(CXX) $(CXXFLAGS_SCAN) -fPIC -shared -o $@ $<

$(HERE)itb_scan_check: $(SCAN_DEPS)
	$(CXX) $(CXXFLAGS_SCAN) $(SAN) -DITB_SCAN_CHECK -o $@ $<

clean:
	rm -f $(HERE)libitb_scan_host.so $(HERE)itb_scan_check

.PHONY: all clean
