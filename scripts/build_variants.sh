#!/bin/bash
# Build timing variants of libgr.so (compile-time -D flags) into build/var/libgr_<name>.so, each by csrc/Makefile (the
# only list of sources and flags) with its own object directory.
# Usage: [VAR_DIR=dir] build_variants.sh name1="-DFOO=1 -DBAR" name2="..."
# (VAR_DIR defaults to build/var, which .gpurunignore keeps off the GPU box: use e.g. VAR_DIR=var to ship them)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
V=$R/${VAR_DIR:-build/var}
mkdir -p $V
pids=()
for spec in "$@"; do
  name=${spec%%=*}; flags=${spec#*=}
  make -s -B -C $R/generalizableracing_amd/csrc -j4 OUT=$V/libgr_$name.so OBJ=$R/build/var_obj/$name EXTRA_FLAGS="$flags" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
