#!/bin/bash
# Build the base side of an A/B run: the kernel source FILE (under csrc/hip) as of git revision REV, compiled with
# the library's own flags (_native.hip_flags() + PER_FILE_FLAGS: no packed FP32) and linked with the tree's current
# objects of every other source, into lib_ab/libqdml_hip_base.so -- where scripts/ab_lib.sh reads it.
# Usage: scripts/build_ab_lib.sh REV conv.hip   (after the in-tree build)
set -eo pipefail
REV=$1; F=$2
R=$(cd "$(dirname "$0")/.." && pwd)
P=$R/quantum_distributed_machine_learning_ris_channel_estimation_amd
T=$(mktemp -d)
git -C "$R" show "$REV:quantum_distributed_machine_learning_ris_channel_estimation_amd/csrc/hip/$F" > "$T/$F"
FLAGS=$(cd "$R" && python -c "from quantum_distributed_machine_learning_ris_channel_estimation_amd import _native as n; print(' '.join(n.hip_flags() + n.PER_FILE_FLAGS.get('$F', [])))")
/opt/rocm/bin/hipcc $FLAGS -c "$T/$F" -o "$T/$F.o"
OBJS=$(ls "$P"/lib/obj/*.o | grep -v "/$F.o\$")
mkdir -p "$R/lib_ab"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$R/lib_ab/libqdml_hip_base.so" $OBJS "$T/$F.o"
rm -rf "$T"
echo "built $R/lib_ab/libqdml_hip_base.so ($F at $REV)"
