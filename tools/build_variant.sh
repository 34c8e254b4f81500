#!/bin/bash
# Build a variant of libtxmom.so with extra flags on ONE source file (the diagnostic builds of DESIGN.md's switch table):
#   bash tools/build_variant.sh <out.so> <source.hip> <flags...>      e.g.  tools/build/libtxmom_timing.so txm_resample_i8t.hip -DTXM_I8T_TIMING
set -e
cd "$(dirname "$0")/.."
OUT=$1; SRC=$2; shift 2
C=thermoextrap_amd/csrc
mkdir -p tools/build
O=tools/build/$(basename "$OUT" .so)_$(basename "$SRC" .hip).o
# the product flags of this file, as thermoextrap_amd/_build.py compiles it
FLAGS=$(python3 -c "import sys; from thermoextrap_amd._build import FLAGS, EXTRA_FLAGS; print(' '.join(FLAGS + EXTRA_FLAGS.get(sys.argv[1], [])))" "$SRC")
/opt/rocm/bin/hipcc $FLAGS "$@" -c $C/$SRC -o $O
OBJS=""
for f in $(python3 -c "from thermoextrap_amd._build import SOURCES; print(' '.join(s[:-4] for s in SOURCES))"); do
  if [ "$f.hip" = "$SRC" ]; then OBJS="$OBJS $O"; else OBJS="$OBJS $C/build/$f.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $OBJS
echo built $OUT
