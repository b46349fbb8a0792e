#!/bin/bash
# build an ablation variant of libdtsim.so: tools/build_variant.sh NAME "-DFOO=1 ..."  ->  lib/libdtsim_NAME.so (units, flags: build.py)
set -e
exec python "$(dirname "$0")/../gym-duckietown_amd/build.py" --variant "$1" $2
