#!/bin/bash
# variant build of the library for A/B experiments: tools/build_variant.sh NAME "-DFLAG=.. -DFLAG2"
# -> csrc/libmgs_NAME.so (objects in /tmp/mgs_var_NAME; the normal build is not touched).  Use with MGS_LIB=<path>.
set -e
NAME=$1; FLAGS=$2
C=$(cd "$(dirname "$0")/../vk_gaussian_splatting_amd/csrc" && pwd)
O=/tmp/mgs_var_$NAME; mkdir -p $O
make -C $C -j8 OBJDIR=$O OUT=libmgs_$NAME.so EXTRA="$FLAGS"
ls -la $C/libmgs_$NAME.so
