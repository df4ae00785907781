#!/bin/bash
# Test infrastructure for tests/test_averaging_ref.py and the GPU averaging
# tests: the CPU restatement of the elastic-averaging and Polyak-Ruppert
# barriers (tests/native/averaging_ref.c), gcc alone.
#   tests/native/libaveraging_ref.so  (git-ignored; travels to the GPU box)
# -ffp-contract=off: every fma is written out, none may be formed or split.
set -euo pipefail
cd "$(dirname "$0")/.."
N=tests/native
gcc -O2 -fPIC -shared -std=c11 -Wall -Wextra -ffp-contract=off -fno-fast-math \
  -o "$N/libaveraging_ref.so.tmp" "$N/averaging_ref.c" -lm
mv "$N/libaveraging_ref.so.tmp" "$N/libaveraging_ref.so"
echo "built $N/libaveraging_ref.so"
