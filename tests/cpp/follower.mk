# The C++ mirror program of the live follower: a g++ host program over libsoundsym_amd.so + ONE HIP runtime, as tests/cpp/Makefile
# builds test_mirror_dtw.  make -C tests/cpp -f follower.mk; tests/test_gpu_mirror_follower.py compares what the program writes
ROOT := $(abspath ../..)
HIPLIB ?= /opt/rocm/lib
HEADERS := $(ROOT)/include/soundsym.hpp $(ROOT)/include/soundsym_amd.h
CXXFLAGS := -std=c++17 -O1 -Wall -Wextra -I$(ROOT)/include
LIBS := -L$(ROOT)/soundsym_amd -lsoundsym_amd -L$(HIPLIB) -lamdhip64 -Wl,-rpath,$(ROOT)/soundsym_amd -Wl,-rpath,$(HIPLIB)
all: test_mirror_follower
test_mirror_follower: test_mirror_follower.cpp $(HEADERS)
	g++ $(CXXFLAGS) $< -o $@ $(LIBS)
clean:
	rm -f test_mirror_follower
.PHONY: all clean
