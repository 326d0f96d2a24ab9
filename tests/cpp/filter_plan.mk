# The dump program of the dtw filter's launch plan: a g++ host program over dtw_filter_plan.hpp alone, no HIP and no library.
# make -C tests/cpp -f filter_plan.mk [OUT=<program>] [EXTRA=-fsanitize=address,undefined]; tests/test_filter_plan.py builds
# and runs it
ROOT := $(abspath ../..)
OUT ?= filter_plan_dump
EXTRA ?=
CXXFLAGS := -std=c++17 -O1 -g -Wall -Wextra -I$(ROOT)/soundsym_amd/csrc $(EXTRA)
all: $(OUT)
$(OUT): filter_plan_dump.cpp $(ROOT)/soundsym_amd/csrc/dtw_filter_plan.hpp
	g++ $(CXXFLAGS) $< -o $@
clean:
	rm -f $(OUT)
.PHONY: all clean
