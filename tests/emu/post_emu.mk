# post_emu.mk -- the rules of every tests/<name>_emu/Makefile: CPU lock-step emulation drivers of the post-decode bodies, test aid
# only.  The including Makefile sets
#   NAME         its directory's name: <NAME>.cpp builds libcbc_<NAME>.so
#   CHECK_MACRO  (optional) -D<CHECK_MACRO> makes <NAME>.cpp a stand-alone program with its own main: `make asan_check` builds it as
#                <NAME>_check under AddressSanitizer / UBSan
#   CHECK_RUN    (optional) a command `make asan_check` runs after building
#   ASAN_LIB     (optional) `make asan` builds libcbc_<NAME>_asan.so
# Header dependencies come from the compiler (-MMD -MP), next to each output as <output>.d.
CXX ?= g++
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wno-unused-function -fPIC -fvisibility=hidden -pthread
SANITIZE = -fsanitize=address,undefined -fno-sanitize-recover=undefined
DEPFLAGS = -MMD -MP -MF $@.d
MK = Makefile ../emu/post_emu.mk

.PHONY: all asan asan_check clean
all: libcbc_$(NAME).so
libcbc_$(NAME).so: $(NAME).cpp $(MK)
	$(CXX) $(CXXFLAGS) $(DEPFLAGS) -shared -o $@ $(NAME).cpp
ifdef CHECK_MACRO
asan_check: $(NAME)_check
	$(CHECK_RUN)
$(NAME)_check: $(NAME).cpp $(MK)
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unused-function $(SANITIZE) -pthread -D$(CHECK_MACRO) $(DEPFLAGS) -o $@ $(NAME).cpp
endif
ifdef ASAN_LIB
asan: libcbc_$(NAME)_asan.so
libcbc_$(NAME)_asan.so: $(NAME).cpp $(MK)
	$(CXX) -O1 -g -std=c++17 $(SANITIZE) -fPIC -pthread $(DEPFLAGS) -shared -o $@ $(NAME).cpp
endif
clean:
	rm -f libcbc_$(NAME).so libcbc_$(NAME)_asan.so $(NAME)_check *.d
-include $(wildcard *.d)
