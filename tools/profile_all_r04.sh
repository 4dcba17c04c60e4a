set -x
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the folder that collects the logs and JSON lines}
bash tools/profile_gpu.sh r04 > $OUT/prof_r04.log 2>&1
bash tools/profile_gpu.sh r04m3 --sampler-mode 3 > $OUT/prof_r04m3.log 2>&1
bash tools/profile_sq.sh r04sq > $OUT/prof_r04sq.log 2>&1
bash tools/profile_sq.sh r04sqm3 --sampler-mode 3 > $OUT/prof_r04sqm3.log 2>&1
bash tools/profile_train_traffic.sh r04train > $OUT/prof_r04train.log 2>&1
bash tools/profile_sq_train.sh r04sqtrain > $OUT/prof_r04sqtrain.log 2>&1
python tools/exp/eps_stress.py > $OUT/eps_stress_r04.txt 2>&1
python tools/bench_latency.py > $OUT/latency_r04.txt 2>&1
python bench.py --full > $OUT/bench_r04.json 2> $OUT/bench_r04.err
python bench.py --full --mode train > $OUT/bench_train_r04.json 2> $OUT/bench_train_r04.err
python bench.py --full --sampler-mode 3 --no-extras > $OUT/bench_r04_mode3.json 2> $OUT/bench_r04_mode3.err
tail -3 $OUT/latency_r04.txt
