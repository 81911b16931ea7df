# tests/native/itb_kvget.mk -- CPU harnesses of the key/value get's ITB walk
# (pomegranate_amd/csrc/itb_kvget.h as plain C++; never part of the product
# library).  Built by __graft_entry__.build(): make -f itb_kvget.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
CXXFLAGS_KVGET = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(abspath $(HERE)../../include)
# itb_kvget_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
KVGET_DEPS = $(HERE)itb_kvget_host.cc $(CSRC)/itb_kvget.h $(CSRC)/itb_find.h $(CSRC)/itb_scan.h \
    $(HERE)../../include/pom_kvget.h $(HERE)../../include/pom_kvlist.h $(HERE)../../include/pom_lookup.h $(HERE)../../include/pom_readdir.h $(HERE)../../include/pom_gc.h

all: $(HERE)libitb_kvget_host.so $(HERE)itb_kvget_check

$(HERE)libitb_kvget_host.so: $(KVGET_DEPS)
	$(CXX) $(CXXFLAGS_KVGET) -fPIC -shared -o $@ $<

$(HERE)itb_kvget_check: $(KVGET_DEPS)
	$(CXX) $(CXXFLAGS_KVGET) $(SAN) -DITB_KVGET_CHECK -o $@ $<

clean:
	rm -f $(HERE)libitb_kvget_host.so $(HERE)itb_kvget_check

.PHONY: all clean
