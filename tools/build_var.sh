#!/bin/bash
# Experiment build of the backend into rust-modem_amd/build/var/<name>/libmodem_hip.so (A/B with
# tools/ab.sh, tools/ab_variants.sh), with the MODEM_VARIANTS_MIN build option (modem_variants.h:
# the BASELINE filters' matrix-core variants only; other filters run on the VALU kernels) plus any
# extra hipcc flags. FULL=1: every variant, as the in-tree library. The Makefile knows the sources;
# this only points it at the variant's own directories.
# Usage: [FULL=1] tools/build_var.sh <name> [hipcc flags...]
set -e
name=$1; shift
cd "$(dirname "$0")/../rust-modem_amd"
d=build/var/$name
MIN=-DMODEM_VARIANTS_MIN; [ "${FULL:-0}" = 1 ] && MIN=
make -s -j"${JOBS:-8}" BUILD=$d/obj LIBDIR=$d EXTRA="$MIN $*" $d/libmodem_hip.so
echo "built $d/libmodem_hip.so"
