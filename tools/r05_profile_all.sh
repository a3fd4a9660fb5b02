#!/bin/bash
# tools/r05_profile_all.sh -- the round-5 evidence set in one GPU-box call (everything lands under gpurun_out/r05_final/; what is
# judged is copied into profiles/ by tools/r05_collect.sh): PMC traffic tables (fp32 batch 32 / 8 / 4, fp16, ResNet18), the default
# bench line, rocprofv3 kernel stats of the same command (fp32, fp16, ResNet18), per-layer tables with the bound each layer sits
# under, the opt-in f32_split runs, the shared-device
# multi-rank runs incl. RCCL through the C-ABI at world 1.
export SI_COMMIT=${SI_COMMIT:-$(git rev-parse --short HEAD 2>/dev/null || echo unknown)}
export TMPDIR=/tmp
O=gpurun_out/r05_final
mkdir -p $O
bash tools/run_traffic.sh r05_final/traffic > $O/traffic_stdout.txt 2>&1
bash tools/run_traffic.sh r05_final/traffic_fp16 --fp16 1 > $O/traffic_fp16_stdout.txt 2>&1
bash tools/run_traffic.sh r05_final/traffic_resnet18 --model resnet18 --batch 64 --size 224 > $O/traffic_resnet18_stdout.txt 2>&1
bash tools/run_traffic.sh r05_final/traffic_b8 --batch 8 > $O/traffic_b8_stdout.txt 2>&1
bash tools/run_traffic.sh r05_final/traffic_b4 --batch 4 > $O/traffic_b4_stdout.txt 2>&1
for t in traffic traffic_fp16 traffic_resnet18 traffic_b8 traffic_b4; do cp $O/$t/traffic.json profiles/$t.json; done
( time python bench.py --full ) > $O/bench_default.json 2> $O/bench_default.err
bash tools/run_rocprof.sh r05_final/prof --min-time 3 > /dev/null 2>&1
python bench.py --full --no-cpu-baseline --no-aux --no-secondary --layers > $O/bench_layers.json 2> $O/layers.txt
for b in 16 8 4 2 1; do python bench.py --full --batch $b --no-cpu-baseline --no-aux --min-time 3 --layers > $O/bench_batch$b.json 2> $O/layers_batch$b.txt; done
python bench.py --full --no-cpu-baseline --no-aux --fp16 1 --layers > $O/bench_fp16.json 2> $O/layers_fp16.txt
SI_CONV_F16_SLAB=0 python bench.py --full --no-cpu-baseline --no-aux --fp16 1 --min-time 3 > $O/bench_fp16_slab0.json 2>/dev/null
bash tools/run_rocprof.sh r05_final/prof_fp16 --fp16 1 --min-time 3 > /dev/null 2>&1
python bench.py --full --no-cpu-baseline --no-aux --model resnet18 --batch 64 --size 224 --layers > $O/bench_resnet18_b64.json 2> $O/layers_resnet18.txt
bash tools/run_rocprof.sh r05_final/prof_resnet18 --model resnet18 --batch 64 --size 224 --min-time 3 > /dev/null 2>&1
python bench.py --full --no-cpu-baseline --no-aux --model resnet18 --batch 64 --size 224 --fp16 1 > $O/bench_resnet18_b64_fp16.json 2>/dev/null
python bench.py --full --no-cpu-baseline --no-aux --model mobilenetv3 --batch 64 --size 224 > $O/bench_mobilenetv3_b64.json 2>/dev/null
python bench.py --full --no-cpu-baseline --no-aux --model mobilenetv3 --batch 64 --size 224 --fp16 1 > $O/bench_mobilenetv3_b64_fp16.json 2>/dev/null
SI_BENCH_SHARE_DEVICE=1 python bench.py --full --gpus 2 --gather p2p --no-cpu-baseline --no-aux --global-batch 32 --min-time 3 > $O/bench_2ranks_shared_device.json 2> $O/bench_2ranks.err
SI_BENCH_SHARE_DEVICE=1 python bench.py --full --gpus 8 --gather p2p --no-cpu-baseline --no-aux --global-batch 32 --min-time 3 > $O/bench_8ranks_shared_device.json 2> $O/bench_8ranks.err
SI_BENCH_FORCE_DIST=1 python bench.py --full --gpus 1 --gather both --no-cpu-baseline --no-aux --no-secondary --min-time 3 > $O/bench_world1_gather_both.json 2> $O/bench_world1_both.err
# opt-in f32_split (fp32 tensors, three fp16 MFMA products per fp32 product): bench line, per-layer table, kernel stats
python bench.py --full --no-cpu-baseline --no-aux --no-secondary --engine-opt f32_split=1 --layers > $O/bench_f32_split.json 2> $O/layers_f32_split.txt
bash tools/run_rocprof.sh r05_final/prof_f32_split --engine-opt f32_split=1 --min-time 3 > /dev/null 2>&1
ls $O
