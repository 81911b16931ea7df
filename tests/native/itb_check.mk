# tests/native/itb_check.mk -- CPU harnesses of the ITB check
# (pomegranate_amd/csrc/itb_check.h as plain C++, and the check's staging
# layout of host_layout.c; never part of the product library).
# Built by __graft_entry__.build(): make -f itb_check.mk -C tests/native
CC ?= gcc
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
INCLUDE := $(abspath $(HERE)../../include)
CXXFLAGS_CHECK = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(INCLUDE)
# itb_check_check and check_layout_check run under AddressSanitizer and UBSan
# where their runtimes link (stand-alone CPU programs; nothing of them is ever
# loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
CHECK_DEPS = $(HERE)itb_check_host.cc $(CSRC)/itb_check.h $(CSRC)/itb_find.h $(CSRC)/itb_scan.h \
    $(INCLUDE)/pom_check.h $(INCLUDE)/pom_lookup.h $(INCLUDE)/pom_readdir.h $(INCLUDE)/pom_gc.h
LAYOUT_SRC = $(CSRC)/host_layout.c
LAYOUT_DEPS = $(HERE)check_layout_check.c $(LAYOUT_SRC) $(CSRC)/host_layout.h

all: $(HERE)libitb_check_host.so $(HERE)itb_check_check $(HERE)check_layout_check

$(HERE)libitb_check_host.so: $(CHECK_DEPS)
	$(CXX) $(CXXFLAGS_CHECK) -fPIC -shared -o $@ $<

$(HERE)itb_check_check: $(CHECK_DEPS)
	$(CXX) $(CXXFLAGS_CHECK) $(SAN) -DITB_CHECK_CHECK -o $@ $<

$(HERE)check_layout_check: $(LAYOUT_DEPS)
	$(CC) -O1 -g -std=gnu11 -Wall -Wextra $(SAN) -I$(CSRC) -I$(INCLUDE) -o $@ $(HERE)check_layout_check.c $(LAYOUT_SRC)

clean:
	rm -f $(HERE)libitb_check_host.so $(HERE)itb_check_check $(HERE)check_layout_check

.PHONY: all clean
