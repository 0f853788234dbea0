#!/bin/bash
# Device assembly of every translation unit of the library (csrc/*.hip), for ISA-identity checks of source-only
# refactors: scripts/isa_dump.sh OUTDIR [extra hipcc flags]; then compare two OUTDIRs kernel by kernel with
# scripts/isa_kernels_diff.py (whichever file a kernel is compiled in), and their budgets with scripts/kernel_regs.py.
# Comments and the compiler's ident/version lines are stripped so only instructions and metadata remain.
set -euo pipefail
out=${1:?outdir}; shift
root=$(cd "$(dirname "$0")/.." && pwd)
src=$root/forging-control_amd/csrc
mkdir -p "$out"
for path in "$src"/*.hip; do
  f=$(basename "$path" .hip)
  /opt/rocm/bin/hipcc -O3 -fno-slp-vectorize --offload-arch=gfx950 -std=c++17 --cuda-device-only -S \
    -I "$root/include" -I "$src" "$@" "$src/$f.hip" -o "$out/$f.s"
  grep -v -E '^\s*(;|//)|\.ident|^\s*$|__hip_cuid_' "$out/$f.s" | sed -e 's/\s*;.*$//' -e 's/\.LBB[0-9]*_/.LBB_/g' -e 's/post_getpc[0-9]*/post_getpc/g' > "$out/$f.clean.s"
done
