#!/bin/bash
# Developer tool (CPU): gpumt_lz4_decompress_blocks_seg's kernels under AddressSanitizer + UndefinedBehaviorSanitizer in a
# stand-alone program (tests/emu/lz4_seg_san.cpp) on the hand-built blocks, the failures in a later segment and the linked runs.
set -e
cd "$(dirname "$0")/.."
A=${TMPDIR:-/tmp}/zmt_lz4_seg_san; mkdir -p $A
PYTHONPATH=$PWD:$PWD/tests:$PWD/tests/golden python -c "import lz4_seg as G; print(G.dump_cases('$A/cases.bin'), 'cases')"
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
H=zstdmt_amd/csrc/hip
for k in lz4_dec pack; do
  g++ -O1 -g -std=c++17 -DZMT_EMU $SAN -Itests/emu -I$H -w -x c++ -c $H/$k.hip -o $A/$k.o &
done
g++ -O1 -g -std=c++17 -DZMT_EMU $SAN -Itests/emu -I$H -w -c tests/emu/emu_runtime.cpp -o $A/emu_runtime.o &
g++ -O1 -g -std=c++17 $SAN -c tests/emu/lz4_seg_san.cpp -o $A/main.o &
wait
g++ $SAN -o $A/lz4_seg_san $A/main.o $A/lz4_dec.o $A/pack.o $A/emu_runtime.o -lpthread
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $A/lz4_seg_san $A/cases.bin
