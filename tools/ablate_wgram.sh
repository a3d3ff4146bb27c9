#!/usr/bin/env bash
# tuning aid: wgram with parts switched off (PAROPT_AMD_WGRAM_ABLATE: 1 no matrix work, 2 no staging either,
# 3 no loads)
set -u
for a in 0 1 3; do
  PAROPT_AMD_WGRAM_ABLATE=$a python tools/microbench.py --tag ab$a --reps 3 | grep wgram
done
