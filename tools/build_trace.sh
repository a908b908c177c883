#!/bin/bash
# trace build of the library (per-workgroup phase stamps in k_project, the sort passes, k_dbin_emit of k_dbin.hip and k_composite of
# k_composite.hip) -> csrc/libmgs_trace.so
# (used by tools/trace_run.sh on the GPU box; objects in /tmp, the normal build is not touched)
set -e
C=$(cd "$(dirname "$0")/../vk_gaussian_splatting_amd/csrc" && pwd)
O=/tmp/mgs_trace_obj; mkdir -p $O
make -C $C -j8 OBJDIR=$O OUT=libmgs_trace.so EXTRA="-DMGS_OS_TRACE -DMGS_PRJ_TRACE -DMGS_DB_TRACE -DMGS_CMP_TRACE"
ls -la $C/libmgs_trace.so
