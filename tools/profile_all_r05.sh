# Runs on the GPU box: every profile summary of round 5 (copied from $OUT/ into profiles/ afterwards)
set -x
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the folder that collects the logs and JSON lines}
bash tools/profile_gpu.sh r05m3 --sampler-mode 3 > $OUT/prof_r05m3.log 2>&1
bash tools/profile_gpu.sh r05m4 --sampler-mode 4 > $OUT/prof_r05m4.log 2>&1
bash tools/profile_sq.sh r05sqm3 --sampler-mode 3 > $OUT/prof_r05sqm3.log 2>&1
bash tools/profile_sq.sh r05sqm4 --sampler-mode 4 > $OUT/prof_r05sqm4.log 2>&1
bash tools/profile_train_traffic.sh r05train > $OUT/prof_r05train.log 2>&1
python bench.py --full > $OUT/bench_r05.json 2> $OUT/bench_r05.err
python bench.py --full --mode train > $OUT/bench_train_r05.json 2> $OUT/bench_train_r05.err
python bench.py --full --sampler-mode 4 --no-extras > $OUT/bench_r05_mode4.json 2> $OUT/bench_r05_mode4.err
python tools/bench_yaml_shapes.py > $OUT/yaml_shapes_r05.jsonl 2> $OUT/yaml_shapes_r05.err
python tools/bench_latency.py > $OUT/latency_r05.txt 2>&1
tail -2 $OUT/latency_r05.txt
