#!/bin/bash
# Builds libpfn_hip.so for gfx950 (MI355X).  Usage: csrc/build.sh [extra hipcc flags]
set -e
cd "$(dirname "$0")"
OUT=../libpfn_hip.so
SRCS="pfn_api.hip gemm.hip gemm_tn.hip attention.hip rowwise.hip bar.hip optim.hip gp_prior.hip gp_fit.hip gp_mcmc.hip bnn_mcmc.hip bnn_svi.hip bnn_svgd.hip bnn_cv.hip xgb_cv.hip catboost_cv.hip tabular.hip logistic.hip gpc.hip mlp_prior.hip stroke_prior.hip class_embed.hip episode.hip"
mkdir -p ../_build
# the headers a source is rebuilt for: the ones every file may include, and those of its own family
headers_of() {
  echo pfn_host.h pfn_device.h ../../include/pfn_hip.h
  case "$1" in
    pfn_api.hip) echo pfn_kernels.h gp_prior.h ;;
    gemm.hip|gemm_tn.hip|attention.hip|rowwise.hip|class_embed.hip) echo pfn_kernels.h ;;
    gp_prior.hip|gp_fit.hip) echo gp_prior.h ;;
    bnn_cv.hip|xgb_cv.hip) echo bnn_device.h fold_device.h ;;
    bnn_*.hip) echo bnn_device.h ;;
    tabular.hip|logistic.hip|gpc.hip|catboost_cv.hip) echo fold_device.h ;;
  esac
}
pids=()
for f in $SRCS; do
  o=../_build/${f%.hip}.o
  stale=""
  for d in "$f" $(headers_of "$f"); do
    if [ ! -f "$o" ] || [ "$d" -nt "$o" ]; then stale=1; fi
  done
  if [ -n "$stale" ]; then
    extra=""
    # attention.hip: no SLP packing -- v_pk_add/mul_f32 beside MFMAs issue slower than the scalar ops they replace
    [ "$f" = attention.hip ] && extra="-fno-slp-vectorize"
    # catboost_cv.hip: no fused multiply-add -- its contract (include/pfn_hip.h) rounds every operation once
    [ "$f" = catboost_cv.hip ] && extra="-ffp-contract=off"
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wno-unused-result $extra "$@" -c "$f" -o "$o" &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT ../_build/pfn_api.o ../_build/gemm.o ../_build/gemm_tn.o ../_build/attention.o ../_build/rowwise.o ../_build/bar.o ../_build/optim.o ../_build/gp_prior.o ../_build/gp_fit.o ../_build/gp_mcmc.o ../_build/bnn_mcmc.o ../_build/bnn_svi.o ../_build/bnn_svgd.o ../_build/bnn_cv.o ../_build/xgb_cv.o ../_build/catboost_cv.o ../_build/tabular.o ../_build/logistic.o ../_build/gpc.o ../_build/mlp_prior.o ../_build/stroke_prior.o ../_build/class_embed.o ../_build/episode.o
echo "built $(realpath $OUT)"
