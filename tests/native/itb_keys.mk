# tests/native/itb_keys.mk -- CPU harnesses of the key/value listing's ITB walk
# (pomegranate_amd/csrc/itb_keys.h as plain C++; never part of the product
# library).  Built by __graft_entry__.build(): make -f itb_keys.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
CXXFLAGS_KEYS = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(abspath $(HERE)../../include)
# itb_keys_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
KEYS_DEPS = $(HERE)itb_keys_host.cc $(CSRC)/itb_keys.h $(CSRC)/itb_dents.h $(CSRC)/itb_scan.h \
    $(HERE)../../include/pom_kvlist.h $(HERE)../../include/pom_readdir.h $(HERE)../../include/pom_gc.h

all: $(HERE)libitb_keys_host.so $(HERE)itb_keys_check

$(HERE)libitb_keys_host.so: $(KEYS_DEPS)
	$(CXX) $(CXXFLAGS_KEYS) -fPIC -shared -o $@ $<

$(HERE)itb_keys_check: $(KEYS_DEPS)
	$(CXX) $(CXXFLAGS_KEYS) $(SAN) -DITB_KEYS_CHECK -o $@ $<

clean:
	rm -f $(HERE)libitb_keys_host.so $(HERE)itb_keys_check

.PHONY: all clean
