#!/bin/bash
# L2 counters of the bf16x3 product kernel under bench.py's headline: hit rate and fabric-side read bytes per launch.
# usage: gemm_bf16x3_pmc.sh TAG [PLANES BAND]   (run from the root of the tree to measure; counters in a run of their own, no tracing)
tag=$1
out=${PMC_OUT:-$(pwd)/build/pmc}/$tag; mkdir -p $out; rm -rf $out/pmc; export TMPDIR=/tmp   # (PMC_OUT: where the runs go; build/ is not tracked)
if [ -n "$2" ]; then export MDHIP_EXPERIMENTS=1 MDHIP_GEMM_BF16X3_PLANES=$2 MDHIP_GEMM_BF16X3_BAND=$3; fi   # (md_options.h: experiment variables are read only behind the gate)
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum --output-format csv -d $out/pmc -- python3 bench.py --gpus 1 --workload cfg2 --steps 3 --warmup 1 > $out/run.log 2>&1 || { tail -5 $out/run.log; exit 1; }
python3 - $out "$tag planes=${2:-default} band=${3:-default}" <<'PY'
import csv, glob, sys, collections
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(sys.argv[1] + '/pmc/**/*_counter_collection.csv', recursive=True):
    for r in csv.DictReader(open(f)):
        if 'bf16x3' in r['Kernel_Name']:
            agg[r['Kernel_Name'].replace('void ', '').replace('(anonymous namespace)::', '').split('(')[0][:40]][r['Counter_Name']].append(float(r['Counter_Value']))
print(sys.argv[2])
for k, c in sorted(agg.items()):
    mean = lambda n: sum(c[n]) / max(len(c[n]), 1)   # noqa: E731
    hit, miss, rd = mean('TCC_HIT_sum'), mean('TCC_MISS_sum'), mean('TCC_EA0_RDREQ_sum')
    # RDREQ x 64 B is FETCH_SIZE's byte count, which tallies the 128-B requests of a wide read at 64 B: doubled
    print("   %-28s launches %3d  hit %12.0f miss %12.0f  hit rate %5.1f %%  RDREQ %12.0f  read bytes per launch %7.3f GiB (RDREQ x 64 B x 2)"
          % (k, len(c['TCC_HIT_sum']), hit, miss, 100 * hit / max(hit + miss, 1), rd, rd * 128 / 2**30))
PY
