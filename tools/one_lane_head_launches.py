"""The prediction head in the last step of a one-lane trace (see tools/one_lane_mask_trace.py): per pyramid level the output convolution (the
launch before each k_head_outputs) and k_head_outputs, then k_select_display / k_coef_at_priors / k_assemble_masks, and the sums.
   python tools/one_lane_head_launches.py <trace dir>"""
import csv
import glob
import os
import sys

trace = max(glob.glob(sys.argv[1] + "/*/*kernel_trace.csv"), key=os.path.getmtime)
rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
FIRST = ("k_import_color_mask", "k_pyramid_level0_color")  # a pass's first kernel: the fused import, or the plain one before k_mask_pre_fused
idx = [i for i, r in enumerate(rows) if any(k in r["Kernel_Name"] for k in FIRST)]
rs = rows[idx[-2]:idx[-1]]
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
span = (int(rs[-1]["End_Timestamp"]) - int(rs[0]["Start_Timestamp"])) / 1e3
busy, end = 0, 0
for r in rs:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    if e > end:
        busy += e - max(s, end)
        end = e
print("step: %.1f us wall, %.1f us with a kernel running, %d launches" % (span, busy / 1e3, len(rs)))
tot = {"output conv": 0.0, "k_head_outputs": 0.0, "k_coef_at_priors": 0.0}
lvl = 0
for i, r in enumerate(rs):
    n = r["Kernel_Name"]
    if "k_head_outputs" in n:
        p = rs[i - 1]
        print("level %d: output conv %8.1f us (%s, grid %s)   k_head_outputs %7.1f us" % (lvl, dur(p), p["Kernel_Name"][:40], p.get("Grid_Size", "?"), dur(r)))
        tot["output conv"] += dur(p)
        tot["k_head_outputs"] += dur(r)
        lvl += 1
    if "k_coef_at_priors" in n:
        print("k_coef_at_priors %7.1f us (grid %s)" % (dur(r), r.get("Grid_Size", "?")))
        tot["k_coef_at_priors"] += dur(r)
    if "k_select_display" in n or "k_assemble_masks" in n:
        print("%s %7.1f us" % (n.split("(")[0][-24:], dur(r)))
for k, v in tot.items():
    print("sum %-18s %9.1f us" % (k, v))
