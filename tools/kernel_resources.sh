#!/bin/bash
# register / spill / scratch / LDS / occupancy table of one .hip source, compiled with the flags of otpose_amd/csrc/Makefile:
#   tools/kernel_resources.sh otpose_amd/csrc/nhwc_conv.hip [filter]
# (code sizes are not in the compiler's remarks: llvm-readelf -s on the unbundled code object has them)
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Xclang -target-feature -Xclang -packed-fp32-ops \
   -Rpass-analysis=kernel-resource-usage -c "$1" -o /tmp/kr.o 2>&1 \
 | grep -E "Function Name|TotalSGPRs:|VGPRs:|AGPRs:|ScratchSize|VGPRs Spill|SGPRs Spill|Occupancy|LDS Size" \
 | sed 's/.*remark: *//; s/\[-Rpass.*//' \
 | awk '/Function Name/{if(n)print n; n=$3} /TotalSGPRs:/{n=n" S="$2} /^ *VGPRs:/{n=n" V="$2} /AGPRs:/{n=n" A="$2} /ScratchSize/{n=n" scratch="$3} /Occupancy/{n=n" occ="$3} /SGPRs Spill/{n=n" sspill="$3} /VGPRs Spill/{n=n" vspill="$3} /LDS Size/{n=n" lds="$4} END{print n}' \
 | c++filt | sed 's/(anonymous namespace):://g; s/(.*) S=/ S=/' | grep -E "${2:-.}"
