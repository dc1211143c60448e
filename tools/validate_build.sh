#!/bin/bash
# tools/validate_build.sh <outdir>: on the GPU box, from the repo root -- the full GPU suite (verbose), the driver's bench line (with --full), the MNIST and
# CelebA-64 workloads, rocprofv3 kernel stats + the PMC traffic record of THIS build (profiles/pmc_traffic.json), and the bench line again with `traffic` filled in.
out=${1:?usage: tools/validate_build.sh <outdir>}
mkdir -p $out
python -m pytest tests -m gpu -q -s > $out/gpu_tests_verbose.log 2>&1
tail -3 $out/gpu_tests_verbose.log
python __graft_entry__.py smoke > $out/smoke.log 2>&1; tail -1 $out/smoke.log
python bench.py --full > $out/bench_cifar.json 2> $out/bench_cifar.err
python bench.py --full --workload mnist_unet_b256_T1000 --no-cpu-baseline > $out/bench_mnist.json 2>&1
python bench.py --full --workload celeba64_unet_b256_T1000 --no-cpu-baseline --steps 20 > $out/bench_celeba64_shard.json 2>&1
python bench.py --full --no-cpu-baseline --no-full-trajectory --clip > $out/bench_cifar_clip.json 2>&1
python bench.py --full --no-cpu-baseline --no-full-trajectory --batch 64 --steps 60 > $out/bench_cifar_b64.json 2>&1
bash tools/profile_bench.sh $out/prof > $out/profile_bench.log 2>&1
cp profiles/pmc_traffic.json $out/pmc_traffic.json
cp profiles/r06/pmc_hbm_traffic.txt $out/pmc_hbm_traffic.txt 2>/dev/null
python bench.py --full --no-cpu-baseline > $out/bench_cifar_with_traffic.json 2>&1
python tools/prof_layers.py --workload cifar10 --batch 1024 > $out/layers_cifar_b1024.txt 2>&1
python tools/prof_layers.py --workload mnist --batch 256 > $out/layers_mnist_b256.txt 2>&1
python -c "
import json
for f in ['bench_cifar','bench_mnist','bench_celeba64_shard','bench_cifar_clip','bench_cifar_b64','bench_cifar_with_traffic']:
    try:
        j=json.loads([l for l in open('$out/%s.json'%f) if l.startswith('{')][-1]); print(f, j['ms_per_step'], j['value'], j['roofline']['frac'], j['roofline']['traffic'], (j['update_kernel'] or {}).get('frac'), (j['update_kernel'] or {}).get('traffic'), (j.get('cpu_baseline') or {}).get('value'), j.get('board_power_w'), j.get('sclk_mhz'), j.get('package_limit_w'))
    except Exception as e: print(f, 'ERR', e)
"
