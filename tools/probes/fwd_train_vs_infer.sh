#!/bin/bash
# the bf16 training forward against the inference forward -- one stamps build each, each run in its own
# process: launch time (HIP events), tile cycles (s_memtime stamps), clock.
#   tools/probes/variant_part.sh st0_infer 0 "-DNERFPP_STAMPS=0"; tools/probes/variant_part.sh st2_train 2 "-DNERFPP_STAMPS=2"
# (The decomposition by component removal -- stores, saves, hand-off, sign words, roles -- is recorded in
# profiles/r06_fwd_train_vs_infer.md; the builds that dropped those components were retired with their switches.)
O=gpurun_out/${1:-fwd_train_vs_infer}; mkdir -p $O
V=$PWD/outdoor_nerf_depth_amd/csrc/build/variants
for rep in 1 2; do
for v in st0_infer st2_train; do
  extra=""; [ $v = st0_infer ] && extra="--infer"
  NERFPP_HIP_LIB=$V/$v.so python tools/probes/stamps_probe.py --what fwd --precision 1 $extra --out $O/${v}_$rep 2>&1 | grep -E "^launch|^tile|^summary" | tr '\n' ' ' | sed "s/^/$v /"; echo
done; done
