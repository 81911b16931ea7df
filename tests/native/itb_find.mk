# tests/native/itb_find.mk -- CPU harnesses of the lookup's ITB walk
# (pomegranate_amd/csrc/itb_find.h as plain C++; never part of the product
# library).  Built by __graft_entry__.build(): make -f itb_find.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
CXXFLAGS_FIND = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(abspath $(HERE)../../include)
# itb_find_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
FIND_DEPS = $(HERE)itb_find_host.cc $(CSRC)/itb_find.h $(CSRC)/itb_scan.h \
    $(HERE)../../include/pom_lookup.h $(HERE)../../include/pom_readdir.h $(HERE)../../include/pom_gc.h

all: $(HERE)libitb_find_host.so $(HERE)itb_find_check

$(HERE)libitb_find_host.so: $(FIND_DEPS)
	$(CXX) $(CXXFLAGS_FIND) -fPIC -shared -o $@ $<

$(HERE)itb_find_check: $(FIND_DEPS)
	$(CXX) $(CXXFLAGS_FIND) $(SAN) -DITB_FIND_CHECK -o $@ $<

clean:
	rm -f $(HERE)libitb_find_host.so $(HERE)itb_find_check

.PHONY: all clean
