#!/bin/bash
# Timing-only builds of conv1x1_sxpc (csrc/seam_pwsx.hip) with parts of its work compiled out (SEAM_SXPC_ABL bits: 1 no row staging,
# 2 no in-loop weight loads, 4 no split VALU, 8 no in-loop A-fragment reads), one small library each under tools/experiments/_lib/
# (kept out of git).  Their outputs are wrong by construction; tools/sxpc_ab.py --abl name=lib times them beside the shipped kernel
# (tools/sxpc64_ab.py --abl: the stem kernel of the same file).
# usage: tools/sxpc_abl_build.sh      (on any machine with hipcc; no GPU needed)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
O=$R/tools/experiments/_lib
mkdir -p $O
for v in "nostage 1" "noweights 2" "nosplit 4" "mfma_epilogue 11"; do
  set -- $v
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I$R/include -I$R/seam-match-rcnn_amd/csrc -DSEAM_SXPC_ABL=$2 -shared \
        $R/seam-match-rcnn_amd/csrc/seam_pwsx.hip -o $O/libsxpc_$1.so
  echo "$O/libsxpc_$1.so (SEAM_SXPC_ABL=$2)"
done
