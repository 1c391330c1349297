#!/bin/bash
# GPU box: build the -DOTP_NHWC_TIMING library variant and print the phase stamps of nhwc_conv_kernel (tools/nhwc_timing.py).
# Only the translation unit whose kernel is stamped is recompiled: nhwc_conv.hip, or nhwc_wgrad.hip for the wgrad form.
# usage: tools/nhwc_timing.sh cin cout h w [wgrad]
set -e
root=${GRAFT_REPO_ROOT:-$(pwd)}
cd $root/otpose_amd/csrc
NOPK="-Xclang -target-feature -Xclang -packed-fp32-ops"
tu=nhwc_conv
[ "$5" = wgrad ] && tu=nhwc_wgrad
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 $NOPK -DOTP_NHWC_TIMING -c $tu.hip -o /tmp/nhwc_t.o 2>/dev/null
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o /tmp/libotp_t.so /tmp/nhwc_t.o $(ls *.o | grep -v "^$tu.o")
cd $root
OTPOSE_HIP_LIB=/tmp/libotp_t.so python tools/nhwc_timing.py "$@"
