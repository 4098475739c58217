# one workload under several settings of one environment switch: VAR=name VALS="a b c" WORKLOAD=ont
set -e
OUT=${OUT:-runs/sweep}
mkdir -p $OUT
w=${WORKLOAD:-ont}
for v in $VALS; do
export $VAR=$v
timeout -k 10 300 python bench.py --full --workload $w --steps 6 --warmup 2 --no-cpu > $OUT/$w.$v.json 2> $OUT/$w.$v.err; python -c "
import json;d=json.load(open('$OUT/$w.$v.json'));r=d['roofline'];print('$w $VAR=$v',d['value'],d['ms_per_step'],r['kernel_ms'],r['seed_kernel_ms'])"
done
