#!/bin/bash
# which object has to be packed-built for the co-residency corruption to appear?  (variants linked by hand from
# babe_amd/build/*.o = product flags and objects built with hipcc defaults; VARIANTS = the directory that holds them,
# one sub-directory with a libbabe_hip.so per variant)
mkdir -p gpurun_out/r4cr
export PARTNERS="${PARTNERS:-bf16p units 64ch,sgu only 64ch,bf16p fwd 64ch,bf16p fwd 256ch}"
for v in "$@"; do
  echo "== $v"
  BABE_HIP_LIB=${VARIANTS:?}/$v/libbabe_hip.so BABE_FFT_MIXED=0 timeout 300 python3 tools/erratum/coresidency_probe.py 2>&1 | grep victim
done > gpurun_out/r4cr/bisect_${TAG:-1}.txt
cat gpurun_out/r4cr/bisect_${TAG:-1}.txt
