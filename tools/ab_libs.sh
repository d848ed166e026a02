#!/bin/bash
# tools/ab_libs.sh ROUNDS "python tools/x.py args" NAME [NAME...] -- the same command on builds of the library
# under kompass-core_amd/lib_ab/NAME/ (tools/build_variant.sh), alternating, ROUNDS times: a same-box A/B.
# A change that grows a context struct alternates every leg of that context, the new one beside them on the builds that
# have it.  For kc_worldmap, grown by the detection of movers (worldmap_time.py --movers needs a build with the entry):
#   for leg in "" --match --points --scan --field --shift --integrate; do
#     tools/ab_libs.sh 3 "python tools/worldmap_time.py $leg" old_parent new; done
#   tools/ab_libs.sh 3 "python tools/worldmap_time.py --movers --integrate" new
# AB_TAIL=N shows the last N lines of every run instead of the last one (mppi_time.py prints a line a shape and leg):
#   AB_TAIL=4 tools/ab_libs.sh 3 "python tools/mppi_time.py --field --no-statement --no-dwa" old_parent new
rounds=$1; cmd=$2; shift 2
root=$(cd "$(dirname "$0")/.." && pwd)
for r in $(seq 1 "$rounds"); do
  for name in "$@"; do
    # (a name that starts with "old_" is a build of an older commit: the binding tolerates entries it lacks)
    old=0; case "$name" in old_*) old=1;; esac
    echo "[$name] $(KOMPASS_HIP_LIB_OLD=$old KOMPASS_HIP_LIB=$root/kompass-core_amd/lib_ab/$name/libkompass_hip.so timeout -k 10 300 $cmd 2>&1 | tail -n "${AB_TAIL:-1}")"
  done
done
