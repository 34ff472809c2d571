#!/bin/bash
# Developer tool (CPU): the three kernels of the segment-parallel chain build under AddressSanitizer +
# UndefinedBehaviorSanitizer in a stand-alone program (tests/emu/win_chain_par_san.cpp) on the shape list of
# tests/win_chain.py: every plane at seg_log 12 and two grids, from exact-size buffers, against the serial kernel's.
set -e
cd "$(dirname "$0")/.."
A=${TMPDIR:-/tmp}/zmt_win_chain_par_san; mkdir -p $A
PYTHONPATH=$PWD:$PWD/tests:$PWD/tests/golden python -c "import win_chain as W; print(W.dump_cases('$A/cases.bin'), 'cases')"
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
H=zstdmt_amd/csrc/hip
KERNELS=$(sed -n 's/^KERNELS := //p' tests/emu/Makefile)
for k in $KERNELS; do
  g++ -O1 -g -std=c++17 -DZMT_EMU $SAN -Itests/emu -I$H -w -x c++ -c $H/$k.hip -o $A/$k.o &
done
g++ -O1 -g -std=c++17 -DZMT_EMU $SAN -Itests/emu -I$H -w -c tests/emu/emu_runtime.cpp -o $A/emu_runtime.o &
g++ -O1 -g -std=c++17 -DZMT_EMU $SAN -Itests/emu -I$H -w -c tests/emu/emu_api.cpp -o $A/emu_api.o &
g++ -O1 -g -std=c++17 $SAN -c tests/emu/win_chain_par_san.cpp -o $A/main.o &
wait
g++ $SAN -o $A/win_chain_par_san $A/main.o $A/emu_api.o $A/emu_runtime.o $(for k in $KERNELS; do echo $A/$k.o; done) -lpthread
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $A/win_chain_par_san $A/cases.bin
