#!/bin/bash
# Builds libzenith_raster from the sources of git revision <rev> into
# zenith_amd/variants/<name>/ (A/B against an earlier commit with tools/ab.sh),
# by this tree's Makefile.
#   tools/build_rev.sh HEAD~1 prev
set -e
rev=$1; name=$2
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d)
git -C "$root" archive "$rev" zenith_amd/csrc include | tar -x -C "$tmp"
out=$root/zenith_amd/variants/$name
make -s -j4 -C "$tmp/zenith_amd" -f "$root/zenith_amd/Makefile" OUT="$out"
rm -rf "$tmp"
echo "$out/libzenith_raster.so"
