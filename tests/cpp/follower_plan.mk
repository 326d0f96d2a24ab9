# The dump program of the live envelope follower's plan: a g++ host program over follower_plan.hpp alone, no HIP and no library.
# make -C tests/cpp -f follower_plan.mk [OUT=<program>] [EXTRA=-fsanitize=address,undefined]; tests/test_follower_plan.py builds
# and runs it
ROOT := $(abspath ../..)
OUT ?= follower_plan_dump
EXTRA ?=
CXXFLAGS := -std=c++17 -O1 -g -Wall -Wextra -I$(ROOT)/soundsym_amd/csrc $(EXTRA)
all: $(OUT)
$(OUT): follower_plan_dump.cpp $(ROOT)/soundsym_amd/csrc/follower_plan.hpp
	g++ $(CXXFLAGS) $< -o $@
clean:
	rm -f $(OUT)
.PHONY: all clean
