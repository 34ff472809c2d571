#!/bin/bash
# Developer tool (CPU): gpumt_brotli_decompress_batch_par's kernels and the record decoders behind them under AddressSanitizer +
# UndefinedBehaviorSanitizer in a stand-alone program (tests/emu/brotli_rec_san.cpp) on own indexed records, foreign flushed
# streams with an index and every tampered record of tests/brotli_rec.py, whole and in slices.
set -e
cd "$(dirname "$0")/.."
A=${TMPDIR:-/tmp}/zmt_brotli_rec_san; mkdir -p $A
PYTHONPATH=$PWD:$PWD/tests:$PWD/tests/golden python -c "import brotli_rec as R; print(R.dump_cases('$A/cases.bin', R.emu_encode), 'batches')"
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
H=zstdmt_amd/csrc/hip
# the record decoders are reached through tests/emu/emu_api.cpp, which names every kernel: all of them are built
KERNELS=$(sed -n 's/^KERNELS := //p' tests/emu/Makefile)
for k in $KERNELS; do
  g++ -O1 -g -std=c++17 -DZMT_EMU $SAN -Itests/emu -I$H -w -x c++ -c $H/$k.hip -o $A/$k.o &
done
for k in emu_runtime emu_api; do
  g++ -O1 -g -std=c++17 -DZMT_EMU $SAN -Itests/emu -I$H -w -c tests/emu/$k.cpp -o $A/$k.o &
done
g++ -O1 -g -std=c++17 $SAN -c tests/emu/brotli_rec_san.cpp -o $A/main.o &
wait
g++ $SAN -o $A/brotli_rec_san $A/main.o $(for k in $KERNELS emu_runtime emu_api; do echo $A/$k.o; done) -lpthread
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $A/brotli_rec_san $A/cases.bin \
  zstdmt_amd/csrc/data/brotli_static.bin
