#!/bin/bash
# usage: tools/build_variant_decode.sh NAME "-DFOO=1 ..."  -> variants/libdabhip_NAME.so (k_decode object rebuilt with the flags, the
# library's other objects as the Makefile lists them: build the library first)
set -e
cd "$(dirname "$0")/../dabtools_amd/csrc"
NAME=$1; FLAGS=$2
OUT=../../variants; mkdir -p $OUT/obj_$NAME
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -w $FLAGS -c k_decode.hip -o $OUT/obj_$NAME/k_decode.o
OBJS=$(make -s print-objs | tr ' ' '\n' | grep -v '^build/k_decode\.o$')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o $OUT/libdabhip_$NAME.so $OUT/obj_$NAME/k_decode.o $OBJS
echo built $OUT/libdabhip_$NAME.so
