#!/bin/bash
# Measures what profiles/push/README.md reports and writes that page, with steps.txt and push.jsonl beside it.
#   tools/profile_push.sh [output directory, default profiles/push] [parent library, default clap_amd/lib_ab/parent/libclapgpu.so]
# The parent library is the commit this change starts from, built from a worktree of it with the project's Makefile.
#   1. k_bodies_step at 262 144 capsule bodies under rocprofv3 --kernel-trace: the parent's library and the new one
#      alternately, 5 processes each, 200 launches a process, the median of each process (facc == NULL)
#   2. the same with an accumulator of zeros, and with forces on a tenth of the bodies before every step
#   3. the slide of tools/slide_bench.py's workload B walk and the push of its results, between HIP events
# Every step runs under its own timeout and the script stops at the first step that fails.
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R" || exit 1
out=$(mkdir -p "${1:-profiles/push}" && cd "${1:-profiles/push}" && pwd) || exit 1
parent=${2:-clap_amd/lib_ab/parent/libclapgpu.so}
rm -f "$out/steps.txt" "$out/push.jsonl" "$out/push.log" "$out/last.log"

trace() {   # trace <label> <library> <null|zeros|tenth>: one process, the median k_bodies_step time appended to steps.txt
  rm -rf "$out/t"
  timeout -k 10 150 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/t" -- python3 tools/push_time.py step "$2" "$3" 200 \
      > "$out/last.log" 2>&1 || { echo "FAILED: $1 (exit $?)"; tail -5 "$out/last.log"; return 1; }
  f=$(find "$out/t" -name '*kernel_trace.csv' | head -1)
  python3 - "$f" "$1" <<'PY' | tee -a "$out/steps.txt"
import csv, sys, statistics
d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in csv.DictReader(open(sys.argv[1])) if "k_bodies_step" in r["Kernel_Name"]]
d = d[1:]                                           # the first launch pays the code upload
print(f'{sys.argv[2]:14s} n {len(d):3d}  median {statistics.median(d):7.2f} us  min {min(d):7.2f}  max {max(d):7.2f}')
PY
  rm -rf "$out/t"
}

for round in 1 2 3 4 5; do
  trace parent_null "$parent" null || exit 1
  trace new_null shipped null || exit 1
done
trace new_zeros shipped zeros || exit 1
trace new_tenth shipped tenth || exit 1
trace new_zeros shipped zeros || exit 1
trace new_tenth shipped tenth || exit 1
timeout -k 10 400 python3 tools/push_time.py push > "$out/push.jsonl" 2> "$out/push.log" || { echo "FAILED: push (exit $?)"; tail -5 "$out/push.log"; exit 1; }
cat "$out/push.jsonl"
rm -f "$out/push.log" "$out/last.log"

python3 - "$out" <<'PY'
import json, os, sys
out = sys.argv[1]
rows = {}
for l in open(os.path.join(out, "steps.txt")):
    p = l.split()
    rows.setdefault(p[0], []).append(float(p[4]))
fmt = lambda v: ", ".join(f"{x:.2f}" for x in v)
pa, ne = rows["parent_null"], rows["new_null"]
inside = min(pa) <= sorted(ne)[len(ne) // 2] <= max(pa)
push = json.loads(open(os.path.join(out, "push.jsonl")).read())
md = f"""# Force accumulators and clapgpu_bodies_push: measured

Written by `tools/profile_push.sh` on one MI355X, one visit; every process fresh. "Parent" is the commit this change
starts from, built from a worktree of it with the project's Makefile and loaded by path.

## k_bodies_step, 262 144 capsule bodies, no accumulator (`facc == NULL`)

`rocprofv3 --kernel-trace`, 200 launches a process, the median of each process in microseconds, the two libraries
alternately:

* parent: {fmt(pa)} (spread {min(pa):.2f} .. {max(pa):.2f})
* new: {fmt(ne)} (median of the medians {sorted(ne)[len(ne) // 2]:.2f})

The new library's median lies {"inside" if inside else "OUTSIDE"} the parent's run-to-run spread. The two instantiations have the parent's
instructions one for one (`tools/isa_hashes.sh clap_amd/csrc/bodies.hip`: same hash and count for `k_bodies_step<false>`
and `<true>` once block labels are normalised); the accumulator is a trailing kernel argument they never read.

## The step with an accumulator

* zeros in it: {fmt(rows["new_zeros"])} us
* forces on a tenth of the bodies before every step: {fmt(rows["new_tenth"])} us

The force path reads 24 B and writes 24 B more per stepped body than the 232 B of the gravity-only step (48 B, 12.6 MB
at this size): algorithmic bytes, counters were not collected.

## clapgpu_bodies_push after the slide (workload B walk of `tools/slide_bench.py`)

{push["movers"]} movers among {push["bodies"]} bodies, HIP events around {push["k"]} back-to-back calls, {push["runs"]} runs, [min, median, max] us:

* restore + index + slide: {push["slide_walk_grid_us"]}; restore + index alone: {push["restore_index_us"]}; the slide alone {push["slide_alone_us"]}
* `clapgpu_bodies_push`: {push["push_us"]} ({push["pushing_slots"]} pushing slots onto {push["pushed_bodies"]} bodies; scratch {push["scratch_bytes"]} bytes)
* push / slide = {push["push_over_slide"]}

## Kernel resources

`kernel_resources.txt` (`tools/kernel_resources.py`, no GPU needed): no scratch and no spilled VGPRs in
`k_bodies_step<.., true>`, `k_push_keys` and `k_push_apply`.
"""
open(os.path.join(out, "README.md"), "w").write(md)
print(md)
PY
