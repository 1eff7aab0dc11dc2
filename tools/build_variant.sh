#!/bin/bash
# Build a variant of libgsr_hip.so for an on-box A/B (tools/ab_multi.sh): tools/build_variant.sh <name> <file.hip> <flags...>
# recompiles ONE kernel file with extra flags behind its own and links it with the in-tree objects of the others
# -> tools/ab/<name>.so.  The object list and every object's flags are the Makefile's (print-objs, EXTRA_FLAGS).
set -e
name=$1; src=$2; shift 2
csrc=mvs_gaussian_splatting_amd/csrc
make -C $csrc -j8 >/dev/null
mkdir -p tools/ab/obj
base=$(basename $src .hip)
# the variant object: the Makefile's rule for it, then moved out of the tree (the next plain make rebuilds the in-tree one)
make -C $csrc -B $base.o EXTRA_FLAGS="-Wno-unused-variable -Wno-unused-const-variable $*" >/dev/null
mv $csrc/$base.o tools/ab/obj/$base.$name.o
objs=""
for o in $(make -s -C $csrc print-objs); do
  if [ $o = $base.o ]; then objs="$objs tools/ab/obj/$base.$name.o"; else objs="$objs $csrc/$o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs -o tools/ab/$name.so
echo "built tools/ab/$name.so"
