#!/bin/bash
# Kernel table of the Swin-T encoder forward on the HIP route (csrc/sd_swin.hip): rocprofv3 --kernel-trace --stats of two forwards of 160 frames
# at 224 x 224 (the first also packs the weights).  The frames are made on the host and copied, so that every kernel in the table belongs to the
# forward.  Usage: tools/profile_swin.sh [OUT_DIR] (default build/prof_swin, git-ignored); writes OUT_DIR/swin_kernel_stats.txt (copied to
# profiles/swin_t_forward_kernel_stats.txt).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${1:-$ROOT/build/prof_swin}" && cd "${1:-$ROOT/build/prof_swin}" && pwd)
cd "$OUT"   # (the profiler's scratch files stay out of the tree)
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/hip -- python3 $ROOT/tools/profile_swin.py > $OUT/hip_prof.log 2>&1
cd $ROOT
{
  echo "# Swin-T encoder forward, 160 frames of 224 x 224, HIP route (eval, no tape): rocprofv3 --kernel-trace --stats of two forwards (the first"
  echo "# packs the weights: token_pack_kernel).  Frames made on the host and copied: every kernel below is the forward's."
  python3 - "$OUT/hip" <<'PY'
import csv, glob, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_stats.csv", recursive=True)[0]
rows = list(csv.DictReader(open(f)))
tot = sum(float(r["TotalDurationNs"]) for r in rows)
print(f"{'kernel':60s} {'calls':>6s} {'total_ms':>9s} {'avg_us':>9s} {'pct':>6s}")
for r in rows:
    print(f"{r['Name'][:60]:60s} {int(r['Calls']):6d} {float(r['TotalDurationNs'])/1e6:9.2f} {float(r['AverageNs'])/1e3:9.1f} {float(r['Percentage']):6.2f}")
print(f"all kernels: {tot/1e6:.2f} ms over {sum(int(r['Calls']) for r in rows)} launches")
bad = [r["Name"] for r in rows if r["Name"].startswith("Cijk") or "miopen" in r["Name"].lower() or "at::" in r["Name"] or "elementwise" in r["Name"].lower()]
print("library GEMM (Cijk_*), MIOpen or ATen kernels:", bad if bad else "none")
PY
} > $OUT/swin_kernel_stats.txt
find $OUT -name "*_kernel_trace.csv" -delete || true
cat $OUT/swin_kernel_stats.txt
