#!/bin/bash
# Build an ablation / experiment twin of the library: scripts/build_variant.sh <name> [extra hipcc flags...]
#   -> wakeword-jupyterlab_amd/csrc/build/ab/lib_<name>.so (git-ignored)
# Use with scripts/ab_kernels.py (interleaved A/B in one process) or WW_LIB_OVERRIDE.
# The source list, the flags and the per-file scheduling strategies are the Makefile's own: its rules run from the variant's object
# directory, so a variant differs from the shipped library only in what it is asked to.  Only sources and headers are searched for in
# csrc (vpath by pattern): a plain VPATH would also find the shipped build/*.o there and compile nothing.
set -e
name=$1; shift
csrc=$(cd "$(dirname "$0")/../wakeword-jupyterlab_amd/csrc" && pwd)
obj=$csrc/build/var_$name
out=$csrc/build/ab/lib_$name.so
mkdir -p "$obj" "$csrc/build/ab"
make -C "$obj" -f "$csrc/Makefile" -j"${MAX_JOBS:-8}" --eval "vpath %.hip $csrc" --eval "vpath %.cpp $csrc" --eval "vpath %.h $csrc" \
     ROOT="$(cd "$csrc/../.." && pwd)" OUT="$out" EXTRA="$*" "$out"
ls -la "$out"
