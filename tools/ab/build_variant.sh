#!/bin/bash
# builds a variant of the solver library into ab/lib_<name>.so:  tools/ab/build_variant.sh <name> [-D... flags for the translation units built from the persistent
# kernel's header and for the host packing that feeds them, uvs_pack.cpp]
# (same flags as __graft_entry__.build, which must have run first: every other unit, i.e. every other *.hip or *.cpp of csrc/, is linked from the
# object file build() made of it; run A/B with tools/ab/run_ab.sh cur ab/lib_<name>.so on the GPU box)
set -e
name=$1; shift
R=$(cd "$(dirname "$0")/../.." && pwd); C=$R/uv-slam_amd/csrc; T=${TMPDIR:-/tmp}/abv_$name; mkdir -p $R/ab $T; rm -f $T/?.o
common="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -w -mllvm -disable-machine-licm"
/opt/rocm/bin/hipcc $common "$@" -c $C/uvs_solver.hip -o $T/a.o &
/opt/rocm/bin/hipcc $common -mllvm -sink-insts-to-avoid-spills "$@" -c $C/uvs_solve512.hip -o $T/b.o &
/opt/rocm/bin/hipcc $common "$@" -c $C/uvs_solve_dstep256.hip -o $T/c.o &
/opt/rocm/bin/hipcc $common "$@" -c $C/uvs_marginalize.hip -o $T/e.o &
/opt/rocm/bin/hipcc $common "$@" -c $C/uvs_large.hip -o $T/f.o &
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -w "$@" -c $C/uvs_pack.cpp -o $T/d.o &
wait
for o in a b c d e f; do [ -f $T/$o.o ] || { echo "a unit of the variant did not compile"; exit 1; }; done
others=""
for src in $C/*.hip $C/*.cpp; do
  obj=${src%.*}.o
  case $obj in $C/uvs_solver.o|$C/uvs_solve512.o|$C/uvs_solve_dstep256.o|$C/uvs_marginalize.o|$C/uvs_large.o|$C/uvs_pack.o) continue;; esac      # rebuilt above
  [ -f $obj ] || { echo "missing $obj: run __graft_entry__.build() first"; exit 1; }
  others="$others $obj"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $T/a.o $T/b.o $T/c.o $T/d.o $T/e.o $T/f.o $others -o $R/ab/lib_$name.so -ldl -pthread
echo built ab/lib_$name.so
