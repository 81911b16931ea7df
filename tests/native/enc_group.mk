# tests/native/enc_group.mk -- CPU harnesses of the grouped encoder's index
# arithmetic and selection rule (pomegranate_amd/csrc/lzo1x_enc_group.h as
# plain C++; never part of the product library).  Built by
# __graft_entry__.build(): make -f enc_group.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
CXXFLAGS_GROUP = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC)
# enc_group_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
GROUP_DEPS = $(HERE)enc_group_host.cc $(CSRC)/lzo1x_enc_group.h

all: $(HERE)libenc_group_host.so $(HERE)enc_group_check

$(HERE)libenc_group_host.so: $(GROUP_DEPS)
	$(CXX) $(CXXFLAGS_GROUP) -fPIC -shared -o $@ $<

$(HERE)enc_group_check: $(GROUP_DEPS)
	$(CXX) $(CXXFLAGS_GROUP) $(SAN) -DENC_GROUP_CHECK -o $@ $<

clean:
	rm -f $(HERE)libenc_group_host.so $(HERE)enc_group_check

.PHONY: all clean
