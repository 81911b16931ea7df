# tests/native/itb_dents.mk -- CPU harnesses of the directory listing's ITB walk
# (pomegranate_amd/csrc/itb_dents.h as plain C++; never part of the product
# library).  Built by __graft_entry__.build(): make -f itb_dents.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
CXXFLAGS_DENTS = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(abspath $(HERE)../../include)
# itb_dents_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
DENTS_DEPS = $(HERE)itb_dents_host.cc $(CSRC)/itb_dents.h $(CSRC)/itb_scan.h \
    $(HERE)../../include/pom_readdir.h $(HERE)../../include/pom_gc.h

all: $(HERE)libitb_dents_host.so $(HERE)itb_dents_check

$(HERE)libitb_dents_host.so: $(DENTS_DEPS)
	$(CXX) $(CXXFLAGS_DENTS) -fPIC -shared -o $@ $<

$(HERE)itb_dents_check: $(DENTS_DEPS)
	$(CXX) $(CXXFLAGS_DENTS) $(SAN) -DITB_DENTS_CHECK -o $@ $<

clean:
	rm -f $(HERE)libitb_dents_host.so $(HERE)itb_dents_check

.PHONY: all clean
