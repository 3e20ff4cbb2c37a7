#!/bin/bash
# round-2 measurement set, part 2: C5 (6x1024) bench + rocprof stats, c2 / c4 / c1 / libri_vgg lines, 2-rank gloo rehearsal on one GPU
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${1:-out}; mkdir -p $O                 # output directory (relative to the repository root)
timeout -k 10 300 python bench.py --full --workload c5 --steps 10 --warmup 3 --no-cpu-baseline > $O/final_bench_c5.json 2> $O/final_bench_c5.err || { tail $O/final_bench_c5.err; exit 5; }
cut -c1-300 $O/final_bench_c5.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/final_prof_c5 -o c5 --output-format csv -- python3 bench.py --workload c5 --steps 4 --warmup 2 --no-cpu-baseline > $O/final_prof_c5.log 2>&1 || exit 6
for w in c2 c4 libri_vgg; do
  timeout -k 10 300 python bench.py --full --workload $w --no-cpu-baseline > $O/final_bench_$w.json 2> $O/final_bench_$w.err || exit 7
  cut -c1-200 $O/final_bench_$w.json
done
timeout -k 10 300 python bench.py --full --workload c1 --cpu-sample-b 8 > $O/final_bench_c1.json 2> $O/final_bench_c1.err || exit 8
cut -c1-200 $O/final_bench_c1.json
LAS_LSTM_NO_XL=1 LAS_DEC_NO_PK=1 LAS_DIST_BACKEND=gloo timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --steps 3 --warmup 1 --no-cpu-baseline 2>$O/final_rank2.err | grep "^{\"metric\"" > $O/final_rank2.json || { tail $O/final_rank2.err; exit 9; }
cut -c1-200 $O/final_rank2.json
