#!/bin/bash
# variant of libmgs.so that differs in k_raster.hip's compile flags only (the other objects are copies of the normal build's):
# tools/build_raster_variant.sh NAME "-DFLAG=.." -> csrc/libmgs_NAME.so.  Use with MGS_LIB=<path>.
set -e
NAME=$1; FLAGS=$2
C=$(cd "$(dirname "$0")/../vk_gaussian_splatting_amd/csrc" && pwd)
make -C $C -j8 >/dev/null
O=/tmp/mgs_rvar_$NAME; mkdir -p $O
cp $C/*.o $O/ && rm -f $O/k_raster.o  # the copies are newer than their sources: only k_raster.o is built, with FLAGS
make -C $C -j8 OBJDIR=$O OUT=libmgs_$NAME.so EXTRA="$FLAGS"
ls -la $C/libmgs_$NAME.so
