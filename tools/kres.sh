#!/bin/bash
# Register / scratch / occupancy figures of the scan (Li0) and resolve (Li1) kernels of the coded, non-wide plan,
# and the biggest basic blocks of the scan kernel (tools/isa_blocks.py).  Cross-compiles: no GPU needed.
# KRES_KERNELS=<extended regex>: the figures of the kernels whose mangled names match instead (nothing else), e.g.
# KRES_KERNELS='format_(copy|sizes|offsets)' for the text path's output stage.
set -e
cd "$(dirname "$0")/.."
mkdir -p /tmp/isa
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -Iinclude -S --cuda-device-only -Rpass-analysis=kernel-resource-usage \
  ${KRES_FLAGS} -o /tmp/isa/x.s cutseq_amd/csrc/cutseq_hip.hip 2>&1 | grep -E -A9 "Function Name: .*(${KRES_KERNELS:-trim_kernelILb1ELb0ELi[01]})" |
  grep -E "Function Name|VGPRs|Scratch|Occupancy|Spill" | sed 's/.*remark: //; s/ \[-Rpass.*//'
[ -n "${KRES_KERNELS}" ] && exit 0
python3 tools/isa_blocks.py /tmp/isa/x.s _ZN5csdev11trim_kernelILb1ELb0ELi0ELi0EEEvNS_5KArgsE ${1:-150}
