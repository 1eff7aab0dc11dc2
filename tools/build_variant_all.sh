#!/bin/bash
# Variant of libgsr_hip.so with EVERY kernel file recompiled with extra flags (a constant of gsr_common.h changed):
#   tools/build_variant_all.sh <name> <flags...>   -> tools/ab/<name>.so
# Objects, flags and link line are the Makefile's, run on a copy of the sources so that the in-tree objects stay as they are.
set -e
name=$1; shift
csrc=mvs_gaussian_splatting_amd/csrc
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
mkdir -p tools/ab $work/pkg/csrc $work/include
cp $csrc/*.hip $csrc/*.h $csrc/Makefile $work/pkg/csrc/
cp include/gsr.h $work/include/
make -C $work/pkg/csrc -j8 OUT=$PWD/tools/ab/$name.so EXTRA_FLAGS="-Wno-unused-variable -Wno-unused-const-variable $*" >/dev/null
echo "built tools/ab/$name.so"
