# tests/native/col_slice.mk -- CPU harnesses of the column reads' decision and
# copy plan (pomegranate_amd/csrc/col_slice.h as plain C++; never part of the
# product library).  Built by __graft_entry__.build(): make -f col_slice.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
CXXFLAGS_SLICE = -O2 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(abspath $(HERE)../../include)
# col_slice_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
SLICE_DEPS = $(HERE)col_slice_host.cc $(CSRC)/col_slice.h

all: $(HERE)libcol_slice_host.so $(HERE)col_slice_check

$(HERE)libcol_slice_host.so: $(SLICE_DEPS)
	$(CXX) $(CXXFLAGS_SLICE) -fPIC -shared -o $@ $<

$(HERE)col_slice_check: $(SLICE_DEPS)
	$(CXX) $(CXXFLAGS_SLICE) $(SAN) -DCOL_SLICE_CHECK -o $@ $<

clean:
	rm -f $(HERE)libcol_slice_host.so $(HERE)col_slice_check

.PHONY: all clean
