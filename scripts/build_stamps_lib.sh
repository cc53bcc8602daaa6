#!/bin/bash
# tuning aid: the library with phase stamps compiled in (-DDSOPP_HIP_STAMPS) into dsopp_amd/lib_stamps/, selected with
# DSOPP_HIP_LIB=$PWD/dsopp_amd/lib_stamps/libdsopp_hip.so (scripts/dbg_*.py); the shipped library carries no stamps.
# The product's own build script with another output directory: same sources, same flags, same link line.
set -euo pipefail
HERE="$(cd "$(dirname "$0")/.." && pwd)"
DSOPP_HIP_OUT="$HERE/dsopp_amd/lib_stamps" DSOPP_HIP_EXTRA_FLAGS="-DDSOPP_HIP_STAMPS ${DSOPP_HIP_EXTRA_FLAGS:-}" bash "$HERE/dsopp_amd/csrc/build.sh"
