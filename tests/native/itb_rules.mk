# tests/native/itb_rules.mk -- the CPU checker of the ITB record rules
# (pomegranate_amd/csrc/itb_rules.h as plain C++; never part of the product
# library).  Built by __graft_entry__.build(): make -f itb_rules.mk -C tests/native
CXX ?= g++
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(abspath $(HERE)../../pomegranate_amd/csrc)
CXXFLAGS_RULES = -O1 -g -std=c++17 -Wall -Wextra -I$(CSRC) -I$(abspath $(HERE)../../include)
# itb_rules_check runs under AddressSanitizer and UBSan where their runtimes
# link (a stand-alone CPU program; nothing of it is ever loaded into Python)
SAN := $(shell echo 'int main(){return 0;}' | $(CXX) -x c++ - -fsanitize=address,undefined \
    -o /dev/null 2>/dev/null && echo -fsanitize=address,undefined -fno-sanitize-recover=undefined)
RULES_DEPS = $(HERE)itb_rules_host.cc $(CSRC)/itb_rules.h $(abspath $(HERE)../../include/pom_itb.h)

all: $(HERE)itb_rules_check

$(HERE)itb_rules_check: $(RULES_DEPS)
	$(CXX) $(CXXFLAGS_RULES) $(SAN) -o $@ $<

# the compress finish as it stood before tmp_cap was honoured: this program's
# report of the overrun (not part of `all`, and no test runs it)
parent: $(HERE)itb_rules_check_parent

$(HERE)itb_rules_check_parent: $(RULES_DEPS)
	$(CXX) $(CXXFLAGS_RULES) $(SAN) -DITB_RULES_PARENT -o $@ $<

clean:
	rm -f $(HERE)itb_rules_check $(HERE)itb_rules_check_parent

.PHONY: all parent clean
