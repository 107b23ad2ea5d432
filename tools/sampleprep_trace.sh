#!/bin/bash
# launches and copies of ONE sampleprep.prepare_batch (N = 8, 512^2, 300 instances per image, bit-packed device masks) from
# rocprofv3 --kernel-trace --memory-copy-trace: everything from the batch's table upload to its device -> host copy.
#   tools/sampleprep_trace.sh OUTDIR        (run on the GPU machine; writes OUTDIR/sampleprep_launches.txt)
set -o pipefail
OUT=${1:?usage: tools/sampleprep_trace.sh OUTDIR}; R=$PWD; mkdir -p "$OUT"; export TMPDIR=/tmp
D=$(mktemp -d /tmp/sptrace.XXXXXX)
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d "$D" -o p -- \
    python "$R/tools/sampleprep_bench.py" --profile-run > "$OUT/sampleprep_trace.log" 2>&1 &&
python - "$D" "$OUT/sampleprep_launches.txt" <<'PY'
import csv, glob, re, sys
d, out = sys.argv[1], sys.argv[2]
ev = []
for r in csv.DictReader(open(glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0])):
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "kernel", re.sub(r"[(<].*", "", r["Kernel_Name"])))
for f in glob.glob(d + "/**/*memory_copy_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy", r.get("Direction") or r.get("Kind", "")))
ev.sort()
first = max(i for i, e in enumerate(ev) if e[3].startswith("sp_image_kernel"))
while first > 0 and ev[first - 1][2] == "copy":          # the table upload in front of the image launch
    first -= 1
rows = ev[first:]
t0 = rows[0][0]
lines = ["# start_us  dur_us  what   (one prepare_batch: N 8, 512 x 512, 300 instances per image, bit-packed device masks)"]
lines += [f"{(s - t0) / 1e3:9.1f} {(e - s) / 1e3:8.1f}  {k:6s} {n}" for s, e, k, n in rows]
count = {}
for _, _, k, n in rows:
    count[(k, n)] = count.get((k, n), 0) + 1
lines += ["# totals"] + [f"# {c:4d} x {k} {n}" for (k, n), c in sorted(count.items())]
open(out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines[-12:]))
PY
rc=$?; rm -rf "$D"; exit $rc
