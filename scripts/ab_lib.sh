#!/bin/bash
# Same-box A/B of two builds of libsdcas on the bench: A = $AB_A (default ab/libsdcas_old.so,
# the previous build), B = $AB_B (default the in-tree library), alternated ABABAB so both see
# the same box and clock history.  Every run keeps the bench's oracle checks (parity sample of
# the steps, the configs[1]/[2] samples, configs[3] files 0 and 15).  Prints sampled / whole /
# step ms, configs[1]/[2] ms and checksum GB/s per run; JSON lines in gpurun_out/$AB_TAG/.
set -u
A=${AB_A:-$PWD/ab/libsdcas_old.so}
B=${AB_B:-$PWD/spacedrive_amd/libsdcas.so}
TAG=${AB_TAG:-ab}
ARGS=${AB_ARGS:---full --no-extras --no-cpu-baseline --config-files 0 --checksum-gib 0 --split-gib 0 --steps 30}
mkdir -p gpurun_out/$TAG
for r in 1 2 3; do
  for v in A B; do
    if [ $v = A ]; then L=$A; else L=$B; fi
    SD_CAS_LIB=$L timeout -k 10 300 python3 bench.py $ARGS > gpurun_out/$TAG/$v$r.json 2> gpurun_out/$TAG/$v$r.err || exit $?
    python3 -c "
import json; d=json.loads(open('gpurun_out/$TAG/$v$r.json').read().strip().splitlines()[-1]); k=d['kernels']
g=d.get('legs', {}); ck=g.get('checksum', {}); rf=d['roofline']
print('$v$r', 'sampled %.3f whole %.3f hash %.3f step %.3f value %.1f M' % (k['sampled_ms'], k['whole_ms'], k['hash_ms'], d['ms_per_step'], d['value']/1e6),
      ' small %.3f sampled1M %.3f' % (g['configs_small']['kernel_ms'], g['configs_sampled']['kernel_ms']) if 'configs_small' in g else '',
      ' sclk %s power %s W' % (rf.get('sclk_mhz_median'), rf.get('board_power_w')),
      ' checksum %.1f GB/s' % ck['GBps'] if ck else '', ' parity mismatches', d['parity']['sample'][1], d['parity']['full'][1])"
  done
done
