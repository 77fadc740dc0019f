#!/bin/bash
# Host-side AddressSanitizer + UBSan run of the in-LDS FFT's plan (vispeech_amd/csrc/fft_plan.h): the header's index math and
# arithmetic, which the kernels of fft.hip call per thread, run item after item by a stand-alone program
# (tools/micro/fft_plan_main.cpp) on frame images of exactly the size a block stages.  Plain C++: needs no GPU, no HIP and
# none of the library.   usage: tools/sanitize_fft_plan.sh [build dir]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-$ROOT/build/sanitize_fft_plan}"
CXX="${CXX:-/opt/rocm/llvm/bin/clang++}"
mkdir -p "$OUT"
"$CXX" -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
  "$ROOT/tools/micro/fft_plan_main.cpp" -o "$OUT/fft_plan"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$OUT/fft_plan"
