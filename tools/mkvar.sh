#!/bin/bash
# tools/mkvar.sh NAME [extra hipcc flags]  -> build/libmbpe_NAME.so  (a variant library for A/B runs: MBPE_LIB=build/libmbpe_NAME.so)
set -e
cd "$(dirname "$0")/.." && mkdir -p build
n=$1; shift
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -fvisibility=hidden "$@" \
  -Iinclude -Iminbpe-cc_amd/csrc -Iminbpe-cc_amd/host \
  $(python3 -c "import __graft_entry__ as g; print(' '.join(g.LIB_SOURCES))") -ldl -o build/libmbpe_$n.so
