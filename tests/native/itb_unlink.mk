# tests/native/itb_unlink.mk -- CPU harnesses of the ITB unlink
# (pomegranate_amd/csrc/itb_unlink.h as plain C++; never part of the product
# library).
# Built by __graft_entry__.build(): make -f itb_unlink.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
INCLUDE := $(abspath $(HERE)../../include)
CXXFLAGS_UNLINK = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(INCLUDE)
# itb_unlink_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
UNLINK_DEPS = $(HERE)itb_unlink_host.cc $(CSRC)/itb_unlink.h $(CSRC)/itb_sweep.h $(CSRC)/itb_split.h \
    $(CSRC)/itb_check.h $(CSRC)/itb_find.h $(CSRC)/itb_scan.h $(INCLUDE)/pom_unlink.h $(INCLUDE)/pom_sweep.h \
    $(INCLUDE)/pom_split.h $(INCLUDE)/pom_check.h $(INCLUDE)/pom_lookup.h $(INCLUDE)/pom_readdir.h $(INCLUDE)/pom_gc.h

all: $(HERE)libitb_unlink_host.so $(HERE)itb_unlink_check

$(HERE)libitb_unlink_host.so: $(UNLINK_DEPS)
	$(CXX) $(CXXFLAGS_UNLINK) -fPIC -shared -o $@ $<

$(HERE)itb_unlink_check: $(UNLINK_DEPS)
	$(CXX) $(CXXFLAGS_UNLINK) $(SAN) -DITB_UNLINK_CHECK -o $@ $<

clean:
	rm -f $(HERE)libitb_unlink_host.so $(HERE)itb_unlink_check

.PHONY: all clean
