#!/bin/bash
# device_isa_digest.sh CHECKOUT [BUILD_DIR] -- one SHA-256 per translation unit of the gfx950 device assembly that
# csrc/build.sh produces, for showing that a refactor compiled to the same device code: run it on the parent's checkout and
# on the branch's, and diff the two outputs.
#
# The checkout's csrc/ and include/ are copied into BUILD_DIR (default: a fresh temporary directory, removed afterwards)
# and built there by the copy's own build.sh, so every file gets its real flags and the checkout is not written to.
# -fuse-cuid=none keeps the __hip_cuid_* symbol from differing between two compiles of the same source; the .file and
# .ident lines (paths, compiler banner) are dropped before hashing.  Prints "name  digest" lines, sorted by name.
set -euo pipefail
[ $# -ge 1 ] || { echo "usage: $0 CHECKOUT [BUILD_DIR]" >&2; exit 2; }
SRC=$(realpath "$1")
if [ $# -ge 2 ]; then
  mkdir -p "$2"
  BUILD=$(realpath "$2")
else
  BUILD=$(mktemp -d)
  trap 'rm -rf "$BUILD"' EXIT
fi
rm -rf "$BUILD/pytheiasfm_amd/csrc" "$BUILD/include"
mkdir -p "$BUILD/pytheiasfm_amd/csrc"
cp -r "$SRC/include" "$BUILD/include"
( cd "$SRC/pytheiasfm_amd/csrc" && cp build.sh *.hip *.h "$BUILD/pytheiasfm_amd/csrc/" )
# without a cuid every object defines the same __hip_cuid_ symbol, so build.sh's final link fails: only its compiles are wanted
THIP_EXTRA_DEFS="-fuse-cuid=none -save-temps=obj" bash "$BUILD/pytheiasfm_amd/csrc/build.sh" >&2 || true
cd "$BUILD/pytheiasfm_amd/csrc"
for f in *.hip; do
  [ -s "_obj/${f%.hip}-hip-amdgcn-amd-amdhsa-gfx950.s" ] || { echo "$f: no device assembly (compile failed?)" >&2; exit 1; }
done
cd _obj
for s in *-hip-amdgcn-amd-amdhsa-gfx950.s; do
  printf '%s  %s\n' "${s%-hip-amdgcn-amd-amdhsa-gfx950.s}" "$(grep -v -e '^[[:space:]]*\.file' -e '^[[:space:]]*\.ident' "$s" | sha256sum | cut -d' ' -f1)"
done
