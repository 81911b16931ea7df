# tests/native/itb_split.mk -- CPU harnesses of the ITB split
# (pomegranate_amd/csrc/itb_split.h as plain C++; never part of the product
# library).
# Built by __graft_entry__.build(): make -f itb_split.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
INCLUDE := $(abspath $(HERE)../../include)
CXXFLAGS_SPLIT = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(INCLUDE)
# itb_split_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
SPLIT_DEPS = $(HERE)itb_split_host.cc $(CSRC)/itb_split.h $(CSRC)/itb_check.h $(CSRC)/itb_find.h $(CSRC)/itb_scan.h \
    $(INCLUDE)/pom_split.h $(INCLUDE)/pom_check.h $(INCLUDE)/pom_lookup.h $(INCLUDE)/pom_readdir.h $(INCLUDE)/pom_gc.h

all: $(HERE)libitb_split_host.so $(HERE)itb_split_check

$(HERE)libitb_split_host.so: $(SPLIT_DEPS)
	$(CXX) $(CXXFLAGS_SPLIT) -fPIC -shared -o $@ $<

$(HERE)itb_split_check: $(SPLIT_DEPS)
	$(CXX) $(CXXFLAGS_SPLIT) $(SAN) -DITB_SPLIT_CHECK -o $@ $<

clean:
	rm -f $(HERE)libitb_split_host.so $(HERE)itb_split_check

.PHONY: all clean
