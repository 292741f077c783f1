#!/bin/bash
# Builds libtheia_hip.so (gfx950) in-tree.  -ffp-contract=off keeps FP64
# arithmetic free of FMA contraction so RANSAC results are bit-reproducible
# against the CPU oracle (built with the same flag).
set -e
cd "$(dirname "$0")"
SRCS=$(ls *.hip)
mkdir -p _obj
OBJS=""
PIDS=""
for f in $SRCS; do
  o=_obj/${f%.hip}.o
  if [ ! -f "$o" ] || [ "$f" -nt "$o" ] || [ -n "$(find . ../../include -maxdepth 1 -name '*.h' -newer "$o")" ]; then
    # the RANSAC / micro-BA files keep the oracle's operation order bit for bit (no FMA contraction); the BA
    # kernels of the large solve are compared at 1e-9 .. 1e-12 and take the FMAs (half the FP64 issue slots)
    # (and reciprocal-based division: 1 ulp, far inside those bounds)
    CONTRACT=off
    case "$f" in ba_fused.hip|ba_fused_intr.hip|ba_kernels.hip) CONTRACT="fast -freciprocal-math -fno-math-errno -fapprox-func" ;; esac
    # the DLS elimination keeps a 93 x 120 matrix in registers; common-code sinking would index it at run time (dls_stage_a.h)
    # (upnp_kernels.hip: the same for its 141 x 149 template)
    case "$f" in dls_kernels.hip|upnp_kernels.hip) CONTRACT="off -mllvm -simplifycfg-sink-common=false" ;; esac
    # ba_inner.hip: the same switch -- sinking the stores of two branches into one store through a pointer phi kept observe_rot()'s
    # residual pair in scratch (24 B per lane, written and read per observation)
    case "$f" in ba_inner.hip) CONTRACT="off -mllvm -simplifycfg-sink-common=false" ;; esac
    # nonlinear_rotations.hip: the same -- the three largest-diagonal branches of the matrix logarithm write different
    # quaternion entries; sunk into one store they kept the whole edge evaluation in scratch (576 B per lane)
    case "$f" in nonlinear_rotations.hip) CONTRACT="off -mllvm -simplifycfg-sink-common=false" ;; esac
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=$CONTRACT -munsafe-fp-atomics \
      -I../../include -I. ${THIP_EXTRA_DEFS:-} -c "$f" -o "$o" &
    PIDS="$PIDS $!"
  fi
  OBJS="$OBJS $o"
done
for p in $PIDS; do wait $p || { echo "compile failed" >&2; exit 1; }; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libtheia_hip.so $OBJS
echo "built $(realpath ../libtheia_hip.so)"
