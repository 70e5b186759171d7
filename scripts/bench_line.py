"""One line of the figures an A/B comparison reads out of a bench.py result: usage  python scripts/bench_line.py TAG RESULT.json
(RESULT.json = the captured stdout of bench.py; its last line is the JSON result)."""
import json
import sys

tag, path = sys.argv[1], sys.argv[2]
r = json.loads(open(path).read().strip().splitlines()[-1])
tw = r.get("timed_window") or {}
prune = r.get("prune") or {}
print(f"{tag}: ms_per_step {r.get('ms_per_step'):.4f}   timed_window.ms_per_step {tw.get('ms_per_step', float('nan')):.4f}   "
      f"prune.ms {prune.get('ms', float('nan')):.4f}   rays/s {r.get('value', float('nan')):,.0f}")
