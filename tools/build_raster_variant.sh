#!/bin/bash
# variant of libmgs.so that differs in ONE object's compile flags (the other objects are copies of the normal build's): k_dbin.o when
# the flags name MGS_DB_*, k_composite.o otherwise (MGS_CMP_*, MGS_SUM_*):
# tools/build_raster_variant.sh NAME "-DFLAG=.." -> csrc/libmgs_NAME.so.  Use with MGS_LIB=<path>.
set -e
NAME=$1; FLAGS=$2
C=$(cd "$(dirname "$0")/../vk_gaussian_splatting_amd/csrc" && pwd)
make -C $C -j8 >/dev/null
case "$FLAGS" in *MGS_DB_*) OBJ=k_dbin.o;; *) OBJ=k_composite.o;; esac
O=/tmp/mgs_rvar_$NAME; mkdir -p $O
cp $C/*.o $O/ && rm -f $O/$OBJ  # the copies are newer than their sources: only $OBJ is built, with FLAGS
make -C $C -j8 OBJDIR=$O OUT=libmgs_$NAME.so EXTRA="$FLAGS"
ls -la $C/libmgs_$NAME.so
