# tests/native/enc_rebase.mk -- CPU harnesses of the encoder's dictionary
# re-base decision (pomegranate_amd/csrc/lzo1x_enc_rebase.h as plain C++; never
# part of the product library).  Built by __graft_entry__.build():
# make -f enc_rebase.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
CXXFLAGS_REBASE = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC)
# enc_rebase_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
REBASE_DEPS = $(HERE)enc_rebase_host.cc $(CSRC)/lzo1x_enc_rebase.h

all: $(HERE)libenc_rebase_host.so $(HERE)enc_rebase_check

$(HERE)libenc_rebase_host.so: $(REBASE_DEPS)
	$(CXX) $(CXXFLAGS_REBASE) -fPIC -shared -o $@ $<

$(HERE)enc_rebase_check: $(REBASE_DEPS)
	$(CXX) $(CXXFLAGS_REBASE) $(SAN) -DENC_REBASE_CHECK -o $@ $<

clean:
	rm -f $(HERE)libenc_rebase_host.so $(HERE)enc_rebase_check

.PHONY: all clean
