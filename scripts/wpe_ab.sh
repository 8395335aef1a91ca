cd "$GRAFT_REPO_ROOT" || exit 2
OUT="${OUT_DIR:-bench_out}/tw"  # OUT_DIR: where the lines go (default bench_out/, git-ignored)
mkdir -p "$OUT"
timeout -k 10 400 python scripts/ab.py --config cfg4 --pipeline fused --rounds 3 base tw7 tw8 > "$OUT/cfg4.jsonl" 2> "$OUT/cfg4.err" || exit $?
timeout -k 10 300 python scripts/ab.py --config cfg2 --pipeline fused --rounds 3 base tw7 tw8 > "$OUT/cfg2.jsonl" 2> "$OUT/cfg2.err" || exit $?
L=cuda-bezier-triangle-raytracer_amd/lib
: > "$OUT/bench.jsonl"
for r in 1 2; do for v in base tw7 tw8; do
  if [ $v = base ]; then lib=$L/libbzr.so; else lib=$L/$v/libbzr.so; fi
  # --full: the line's frame_verified (the last frame against the oracle digests) is read below
  BZR_LIBRARY=$PWD/$lib timeout -k 10 240 python bench.py --full --cpu-baseline off > "$OUT/one.log" 2>&1 || exit $?
  grep '^{' "$OUT/one.log" | python3 -c "
import json,sys; d=json.loads(sys.stdin.read()); print(json.dumps({'variant':'$v','rep':$r,'mrays_s':d['value'],'ms_per_step':d['ms_per_step'],'verified':d['config']['frame_verified']['oracle_digests']['ok']}))" >> "$OUT/bench.jsonl"
done; done
