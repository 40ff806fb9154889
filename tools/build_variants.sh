#!/bin/bash
# Build named variants of libdsp_frontend.so for kernel A/B runs: tools/build_variants.sh name "flags" [name "flags" ...]
# -> dsp-speech-recognition_amd/lib/variants/<name>.so, each from objects of its own (lib/obj/variants/<name>/).
set -e
cd "$(dirname "$0")/../dsp-speech-recognition_amd/csrc"
mkdir -p ../lib/variants
while [ $# -gt 1 ]; do
  name=$1; flags=$2; shift 2
  ( make -j2 LIBNAME="variants/$name.so" EXTRA_CXXFLAGS="$flags" 2>&1 | grep -E "error|warning: v" ; echo "built $name" ) &
  while [ $(jobs -r | wc -l) -ge 4 ]; do sleep 1; done
done
wait
