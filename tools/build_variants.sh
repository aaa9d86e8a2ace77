#!/bin/bash
# Build kernel-experiment variants of liblab4d_hip.so into build/abl/: one per argument; BASE = no define, WSABL_NOST = -DLAB4D_WSABL_NOST,
# ABL_WGRAD_L2 = -DLAB4D_ABL_WGRAD_L2 (the two timing-only ablations of DESIGN.md section 8: their results are WRONG).
#   usage: tools/build_variants.sh BASE WSABL_NOST ABL_WGRAD_L2
#   then on the GPU box:   for v in build/abl/lib_*.so; do LAB4D_ALLOW_EXPERIMENT_BUILD=1 LAB4D_SO_PATH=$v python tools/bench_chain.py; done
cd "$(dirname "$0")/.."
mkdir -p build/abl
for v in "$@"; do
  case "$v" in
    BASE) X="" ;;
    WSABL_NOST|ABL_WGRAD_L2) X="-DLAB4D_$v" ;;
    *) echo "unknown variant $v (BASE, WSABL_NOST, ABL_WGRAD_L2)"; continue ;;
  esac
  LAB4D_HIPCC_EXTRA="$X" LAB4D_SO_PATH=$PWD/build/abl/lib_$v.so LAB4D_BUILD_DIR=$PWD/build/abl/obj_$v \
    python -c "from lab4d_amd import _lib; _lib.build(verbose=False)" || echo "FAIL $v"
done
ls -la build/abl/
