#!/bin/bash
# Timing-only builds of conv3x3_wino24sx (csrc/seam_wino24sx.hip) with parts of its work compiled out (SEAM_W24SX_ABL bits: 1 no
# in-loop patch requests / LDS stores, 2 no in-loop weight loads, 8 no in-loop transform + split VALU, 16 no epilogue arithmetic), one
# small library each under tools/experiments/_lib/ (kept out of git).  Their outputs are wrong by construction;
# tools/w24sx_ab.py --abl name=lib times them beside the shipped kernel.
# usage: tools/w24sx_abl_build.sh      (on any machine with hipcc; no GPU needed)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
O=$R/tools/experiments/_lib
mkdir -p $O
for v in "nopatch 1" "noweights 2" "novalu 8" "mfma_epilogue 11"; do
  set -- $v
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I$R/include -I$R/seam-match-rcnn_amd/csrc -DSEAM_W24SX_ABL=$2 -shared \
        $R/seam-match-rcnn_amd/csrc/seam_wino24sx.hip -o $O/libw24sx_$1.so
  echo "$O/libw24sx_$1.so (SEAM_W24SX_ABL=$2)"
done
