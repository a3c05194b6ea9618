#!/bin/bash
# build tools/_bin/tgemm_base: the training GEMM kernels with their phase stamps (GVL_WG_STAMPS)
root=$(cd $(dirname $0)/../.. && pwd)
mkdir -p $root/tools/_bin
build() { /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -I $root/include -I $root/gvl_amd/csrc $2 -o $root/tools/_bin/tgemm_$1 $root/tools/ubench/tgemm_bench.hip 2>&1 | grep -v warning | grep -i "error" ; }
build base "-DGVL_WG_STAMPS"
ls -la $root/tools/_bin/tgemm_base
