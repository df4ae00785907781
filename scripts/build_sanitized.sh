#!/bin/bash
# Host-side AddressSanitizer + UndefinedBehaviorSanitizer build of the C-ABI
# library sources linked into a plain-C driver (tests/native/abi_driver.c).
# Every -fsanitize= on the hipcc line sits right after -Xarch_host: device
# code is not instrumented (no GPU ASan on this pool).  Output:
# tests/native/abi_driver_asan (git-ignored; it travels to the GPU box with
# the tree).  Run here, on the CPU.
set -euo pipefail
cd "$(dirname "$0")/.."
OUT=tests/native/abi_driver_asan
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
/opt/rocm/lib/llvm/bin/clang -c -O1 -g -std=c11 -fno-omit-frame-pointer -fsanitize=address,undefined \
  -I include -o "$TMP/abi_driver.o" tests/native/abi_driver.c
# One object per source, compiled side by side ($MAX_JOBS at a time, else one per CPU, 16 at the most), then one link.
SRCS="crossbow_amd/csrc/context.hip crossbow_amd/csrc/sync_steps.hip crossbow_amd/csrc/sma_kernels.hip crossbow_amd/csrc/averaging_kernels.hip crossbow_amd/csrc/sma_seam.hip crossbow_amd/csrc/stats_kernels.hip crossbow_amd/csrc/variable_rate_kernels.hip crossbow_amd/csrc/clip_kernels.hip crossbow_amd/csrc/task_barrier_kernels.hip crossbow_amd/csrc/task_barrier_variables_kernels.hip crossbow_amd/csrc/task_barrier_clipped_kernels.hip crossbow_amd/csrc/task_barrier_clipped_variables_kernels.hip crossbow_amd/csrc/task_elastic_kernels.hip crossbow_amd/csrc/task_ssgd_kernels.hip crossbow_amd/csrc/task_elastic_clipped_variables_kernels.hip crossbow_amd/csrc/task_elastic_clipped_kernels.hip crossbow_amd/csrc/task_elastic_variables_kernels.hip"
JOBS=${MAX_JOBS:-$(nproc)}
[ "$JOBS" -gt 16 ] && JOBS=16
export TMP
printf '%s\n' $SRCS | xargs -P "$JOBS" -I{} sh -c \
  '/opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -Xarch_host -gline-tables-only -std=c++17 -ffp-contract=off -fno-omit-frame-pointer \
     -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
     -I include -c -o "$TMP/$(basename "$1" .hip).o" "$1"' sh {}
OBJS=$(for f in $SRCS; do printf '%s ' "$TMP/$(basename "$f" .hip).o"; done)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
  -o "$OUT.tmp" $OBJS "$TMP/abi_driver.o" \
  -lrccl -lrocprofiler-sdk-roctx -lpthread
mv "$OUT.tmp" "$OUT"
echo "built $OUT"
