#!/bin/bash
# Build librtmi.so with extra compile definitions into OUT (A/B experiments, container side): the
# library's own Makefile, its objects in a directory of their own.
# usage: bash profiles/build_variant.sh OUT.so -DNAME=VALUE ...
set -e
OUT=$(realpath -m "$1"); shift
SRC=${SRC_DIR:-$(dirname "$(realpath "$0")")/../pathtracer.cl_amd/csrc}
B=$(mktemp -d)
make -s -j"${JOBS:-16}" -C "$SRC" OUT="$OUT" BUILD="$B" EXTRA="$*" "$OUT"
rm -rf "$B"
echo built "$OUT"
