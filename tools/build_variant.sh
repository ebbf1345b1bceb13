#!/bin/bash
# Build a variant of libmvr_hip.so with extra -D flags for mvr_cull.hip / mvr_grid.hip / mvr_reduce.hip / mvr_ctx.hip / mvr_align.hip (tuning and diagnostics):
#   tools/build_variant.sh stamp -DMVR_STAMP      -> build/libmvr_hip_stamp.so   (in-kernel cycle stamps; run with MVR_STAMP_DUMP=1)
#   tools/build_variant.sh w6 -DMVR_CULL_WAVES=6  -> build/libmvr_hip_w6.so
# Select it with MVR_LIB_VARIANT=<name> (the Python package then loads build/libmvr_hip_<name>.so; experiments only).
set -e
cd "$(dirname "$0")/.."
name=$1; shift
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -fno-fast-math -fno-slp-vectorize $* -Iinclude -Imulti-view-registration_amd/csrc"
mkdir -p build/obj
variant="mvr_cull mvr_ctx mvr_align mvr_grid mvr_reduce"
objs=""
for v in $variant; do
  /opt/rocm/bin/hipcc $F -x hip -c multi-view-registration_amd/csrc/$v.hip -o build/obj/${v}_$name.o &
  objs="$objs build/obj/${v}_$name.o"
done
wait
# every other object comes from the regular build (python __graft_entry__.py)
for o in build/obj/*.hip.o build/obj/*.cpp.o build/obj/*.c.o; do
  case " $variant " in *" $(basename "$o" .hip.o) "*) ;; *) objs="$objs $o" ;; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/libmvr_hip_$name.so $objs -lm -ldl -lpthread
ls -la build/libmvr_hip_$name.so
