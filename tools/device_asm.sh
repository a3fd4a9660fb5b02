#!/bin/bash
# tools/device_asm.sh <outdir> [defines] -- gfx950 device assembly of every HIP source, with build.py's flags:
# writes <outdir>/<file>.s and prints one "sha256  file" line per source.  A refactor that must not move the device
# code runs this on both trees and compares the directories (diff -r).  [defines]: e.g. -DSI_EXPERIMENT, -DSI_DIAG_STAMPS.
# -fuse-cuid=none: the compilation-unit id is a hash of the source's absolute path, and its symbol would make two
# checkouts of the same tree differ.  Run from the repository root.  SI_ASM_JOBS: compiles in flight (default 8).
set -u
OUT=${1:?usage: tools/device_asm.sh <outdir> [defines]}; shift
mkdir -p "$OUT" || exit 1
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
export OUT HIPCC SI_ASM_DEFS="$*"
ls simpleinfer_amd/csrc/hip/*.hip | xargs -P "${SI_ASM_JOBS:-8}" -I{} sh -c \
  '$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude -Isimpleinfer_amd/csrc/hip -fuse-cuid=none $SI_ASM_DEFS --cuda-device-only -S "$1" -o "$OUT/$(basename "$1" .hip).s"' _ {} || exit 1
(cd "$OUT" && sha256sum *.s)
