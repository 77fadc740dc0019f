#!/bin/bash
# Host-side AddressSanitizer + UBSan run of the isolated-mode entry points' argument validation: the library's sources and
# a stand-alone program (tools/micro/isolated_args_main.cpp) compiled with -Xarch_host -fsanitize=address,undefined into ONE
# executable, run on the CPU.  Needs no GPU and launches no kernel.   usage: tools/sanitize_isolated_args.sh [build dir]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-$ROOT/build/sanitize_isolated}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
mkdir -p "$OUT"
SRC="$ROOT/vispeech_amd/csrc"
FLAGS="-O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Wno-unused-function -Xclang -target-feature -Xclang -packed-fp32-ops"
objs=()
for f in "$SRC"/*.hip "$SRC"/weights.cpp; do
  o="$OUT/$(basename "$f").o"
  [ "$o" -nt "$f" ] || "$HIPCC" $FLAGS -x hip -c "$f" -o "$o" &
  objs+=("$o")
  while [ "$(jobs -r | wc -l)" -ge "${JOBS:-8}" ]; do wait -n; done
done
wait
"$HIPCC" $FLAGS -x hip -c "$ROOT/tools/micro/isolated_args_main.cpp" -o "$OUT/main.o"
"$HIPCC" --offload-arch=gfx950 -fsanitize=address,undefined "${objs[@]}" "$OUT/main.o" -o "$OUT/isolated_args"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$OUT/isolated_args"
