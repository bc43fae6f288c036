#!/bin/bash
# developer A/B: a second copy of the library + kbench, into gligen_amd/build/var_NAME/ (git-ignored, travels to the GPU box):
#   tools/build_variant.sh NAME [-D...]       this tree with the GEMM's units (gemm_u.hip, gemm_halo.hip, gemm_wide.hip, gemm_basic.hip,
#                                             gemm.hip: GEMM_UNITS of gligen_amd/build.py) compiled under extra flags, side by side
#   tools/build_variant.sh NAME SRC_TREE      another tree (a checkout of another commit), built by its own gligen_amd/build.py:
#                                             its source list and per-file flags are its own (the library inside SRC_TREE is (re)built)
# tools/gpu_run.sh lib gligen_amd/build/var_NAME swaps it in.
set -e
name=$1; shift
tree=$PWD
if [ -n "$1" ] && [ -d "$1" ]; then tree=$1; shift; fi
out=gligen_amd/build/var_$name
mkdir -p $out
if [ "$tree" = "$PWD" ]; then
  F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -I $tree/include"
  python -m gligen_amd.build > /dev/null
  units=$(python -c "from gligen_amd.build import GEMM_UNITS; print(' '.join(GEMM_UNITS))")
  objs=$(ls gligen_amd/build/*.hip.o)
  pids=
  for u in $units; do
    hipcc $F "$@" -c gligen_amd/csrc/$u -o $out/$u.o & pids="$pids $!"
    objs=$(echo "$objs" | grep -v "/$u.o\$")
  done
  for p in $pids; do wait $p; done
  hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libgligen_amd.so $(for u in $units; do echo $out/$u.o; done) $objs
  hipcc $F $tree/gligen_amd/csrc/kbench.hip -o $out/kbench -L $out -lgligen_amd '-Wl,-rpath,$ORIGIN'
else
  if [ $# -gt 0 ]; then echo "build_variant.sh: extra flags apply to this tree only, not to SRC_TREE (got: $*)" >&2; exit 2; fi
  ( cd $tree && python -m gligen_amd.build > /dev/null )
  cp $tree/gligen_amd/libgligen_amd.so $tree/gligen_amd/build/kbench $out/
fi
ls -la $out/kbench $out/libgligen_amd.so
