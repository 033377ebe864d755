# Round validation on an MI355X box:  bash tools/scripts/round_run.sh [output folder, from the repository root; default round_out]
# full GPU suite, smoke, the driver-style bench, then the profile passes behind profiles/ (render with
# tools/scripts/render_profiles.sh <output folder>/rprof r0N_x afterwards)
cd "$(dirname "$0")/../.."; O=${1:-round_out}; mkdir -p $O
timeout 900 python -m pytest tests -m gpu -x -q > $O/round_pytest.log 2>&1; tail -2 $O/round_pytest.log
timeout 120 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
for i in 1 2 3 4 5; do timeout 120 python bench.py --full --steps 20 --warmup 5 --no-extras --no-cpu-baseline 2>/dev/null | python -c "
import sys,json
d=json.loads([l for l in sys.stdin.read().splitlines() if l.startswith('{')][-1]); print(d['ms_per_step'], d['encode_paths']['two_kernels_ms'], d['encode_paths']['fused_ms'])"; done
timeout 600 python bench.py --full --steps 20 --warmup 5 > $O/round_bench.json 2> $O/round_bench.err
bash tools/scripts/profile_round.sh $O/rprof > $O/round_prof.log 2>&1
python - $O <<'PY'
import json, os, sys
for f in (os.path.join(sys.argv[1], "round_bench.json"), os.path.join(sys.argv[1], "rprof", "stats.log")):
    txt = open(f).read()
    d = json.loads([l for l in txt.splitlines() if l.startswith("{")][-1])
    print(f, d["ms_per_step"], d["value"], d["roofline"]["frac"], d.get("encode_paths", {}).get("two_kernels_ms"), d.get("seeds", {}).get("median"))
PY
