# tests/native/gc_merge.mk -- CPU harnesses of the garbage collector's range
# merge (pomegranate_amd/csrc/gc_merge.h as plain C++, gc_fold.c and host_layout.c as plain C;
# never part of the product library).  Built by __graft_entry__.build():
# make -f gc_merge.mk -C tests/native
# GC_MERGE_INC=-I<dir>, OUT=<dir>/: a gc_merge.h found in <dir> takes the
# header's place and the products go to <dir> (tests/test_gc_merge.py builds the
# harnesses against deliberately wrong rules that way)
CC ?= gcc
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
OUT ?= $(HERE)
GC_MERGE_INC ?=
CXXFLAGS_MERGE = -O2 -g -std=c++17 -Wall -Wextra $(GC_MERGE_INC) -I$(CSRC) -I$(abspath $(HERE)../../include)
CFLAGS_FOLD = -O2 -g -std=gnu11 -Wall -Wextra -I$(CSRC) -I$(abspath $(HERE)../../include)
# gc_merge_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
MERGE_DEPS = $(HERE)gc_merge_host.cc $(CSRC)/gc_merge.h $(CSRC)/gc_fold.c $(CSRC)/gc_fold.h \
    $(CSRC)/host_layout.c $(CSRC)/host_layout.h $(HERE)../../include/pom_gc.h

all: $(OUT)libgc_merge_host.so $(OUT)gc_merge_check

$(OUT)libgc_merge_host.so: $(MERGE_DEPS)
	$(CC) $(CFLAGS_FOLD) -fPIC -c $(CSRC)/gc_fold.c -o $(OUT)gc_fold_host.o
	$(CXX) $(CXXFLAGS_MERGE) -fPIC -shared -o $@ $(HERE)gc_merge_host.cc $(OUT)gc_fold_host.o
	rm -f $(OUT)gc_fold_host.o

$(OUT)gc_merge_check: $(MERGE_DEPS)
	$(CC) $(CFLAGS_FOLD) $(SAN) -c $(CSRC)/gc_fold.c -o $(OUT)gc_fold_check.o
	$(CC) $(CFLAGS_FOLD) $(SAN) -c $(CSRC)/host_layout.c -o $(OUT)gc_layout_check.o
	$(CXX) $(CXXFLAGS_MERGE) $(SAN) -DGC_MERGE_CHECK -o $@ $(HERE)gc_merge_host.cc $(OUT)gc_fold_check.o \
	    $(OUT)gc_layout_check.o
	rm -f $(OUT)gc_fold_check.o $(OUT)gc_layout_check.o

clean:
	rm -f $(OUT)libgc_merge_host.so $(OUT)gc_merge_check $(OUT)gc_fold_host.o $(OUT)gc_fold_check.o $(OUT)gc_layout_check.o

.PHONY: all clean
