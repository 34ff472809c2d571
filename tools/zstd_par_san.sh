#!/bin/bash
# Developer tool (CPU): gpumt_zstd_decompress_blocks_par's kernels under AddressSanitizer + UndefinedBehaviorSanitizer in a
# stand-alone program (tests/emu/zstd_par_san.cpp) on the hand-built frames at every cut and on damaged streams.
set -e
cd "$(dirname "$0")/.."
A=${TMPDIR:-/tmp}/zmt_par_san; mkdir -p $A
PYTHONPATH=$PWD:$PWD/tests:$PWD/tests/golden python -c "import zstd_par as R; print(R.dump_cases('$A/cases.bin'), 'cases')"
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
H=zstdmt_amd/csrc/hip
for k in zstd_dec zstd_dec_seq; do
  g++ -O1 -g -std=c++17 -DZMT_EMU $SAN -Itests/emu -I$H -w -x c++ -c $H/$k.hip -o $A/$k.o &
done
g++ -O1 -g -std=c++17 -DZMT_EMU $SAN -Itests/emu -I$H -w -c tests/emu/emu_runtime.cpp -o $A/emu_runtime.o &
g++ -O1 -g -std=c++17 $SAN -c tests/emu/zstd_par_san.cpp -o $A/main.o &
wait
g++ $SAN -o $A/zstd_par_san $A/main.o $A/zstd_dec.o $A/zstd_dec_seq.o $A/emu_runtime.o -lpthread
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $A/zstd_par_san $A/cases.bin
