# varpaths_emu.mk -- libcbc_emu_varpaths.so: the encoder emulation of emu_encode.cpp with the counters of var_code compiled in
# (emu_varpaths.cpp; test aid only).  make -C tests/emu -f varpaths_emu.mk
CXX ?= g++
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wno-unused-function -fPIC -fvisibility=hidden -pthread
CSRC = ../../cbc_amd/csrc

.PHONY: all clean
all: libcbc_emu_varpaths.so
libcbc_emu_varpaths.so: emu_varpaths.cpp emu_encode.cpp wave_emu.h varpaths_emu.mk $(CSRC)/cbc_encode_body.h $(CSRC)/cbc_decode_body.h $(CSRC)/cbc_plan.h $(CSRC)/cbc_stream_body.h $(CSRC)/cbc_long_body.h $(CSRC)/cbc_tok_core.h ../../include/cbc_gpu.h
	$(CXX) $(CXXFLAGS) -shared -o $@ emu_varpaths.cpp
clean:
	rm -f libcbc_emu_varpaths.so
