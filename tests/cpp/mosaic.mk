# The C++ mirror program of the mosaic: a g++ host program over libsoundsym_amd.so + ONE HIP runtime, as
# tests/cpp/cover.mk builds test_mirror_cover.  make -C tests/cpp -f mosaic.mk; tests/test_gpu_mirror_mosaic.py compares
# what the program writes
ROOT := $(abspath ../..)
HIPLIB ?= /opt/rocm/lib
HEADERS := $(ROOT)/include/soundsym.hpp $(ROOT)/include/soundsym_amd.h
CXXFLAGS := -std=c++17 -O1 -Wall -Wextra -I$(ROOT)/include
LIBS := -L$(ROOT)/soundsym_amd -lsoundsym_amd -L$(HIPLIB) -lamdhip64 -Wl,-rpath,$(ROOT)/soundsym_amd -Wl,-rpath,$(HIPLIB)
all: test_mirror_mosaic
test_mirror_mosaic: test_mirror_mosaic.cpp $(HEADERS)
	g++ $(CXXFLAGS) $< -o $@ $(LIBS)
clean:
	rm -f test_mirror_mosaic
.PHONY: all clean
