#!/bin/bash
# A/B library: tools/build_variant.sh <name> <file.hip> [-DFLAGS...] -> mcmc_amd/libmi_<name>.so (same objects, one TU recompiled)
set -e
cd "$(dirname "$0")/../mcmc_amd/csrc"
NAME=$1; TU=$2; shift 2
FLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -Wall -Wno-unused-function -I../../include/mi_mcmc_engine"
/opt/rocm/bin/hipcc $FLAGS "$@" -c -o build/${TU%.hip}_$NAME.o $TU
BASE=""
for s in $(make -s print-src); do          # the Makefile's SRC: the library's translation units
  if [ "$s" = "$TU" ]; then BASE="$BASE build/${s%.hip}_$NAME.o"; else BASE="$BASE build/${s%.hip}.o"; fi
done
/opt/rocm/bin/hipcc $FLAGS -shared -o ../libmi_$NAME.so $BASE
echo built ../libmi_$NAME.so
