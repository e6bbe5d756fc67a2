# throughput vs. (batch, streams); prints value and ms/step (bench lines and stderr kept in $OUT, default: a new temporary directory)
out=${OUT:-$(mktemp -d)}
for cfg in "4096 4" "8192 8" "8192 4" "6144 6" "4096 8"; do
  set -- $cfg
  timeout -k 10 200 python bench.py --batch $1 --streams $2 --steps 10 --warmup 2 --no-cpu-baseline > $out/ss_$1_$2.json 2>$out/ss_$1_$2.err || { echo "fail $cfg"; tail -3 $out/ss_$1_$2.err; continue; }
  python - <<PY
import json
d = json.loads(open("$out/ss_$1_$2.json").read().strip().splitlines()[-1])
print("$1 $2", d["value"], d["ms_per_step"], d["roofline"]["launch_ms"])
PY
done
