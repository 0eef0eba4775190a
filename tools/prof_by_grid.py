"""Per (kernel, grid, workgroup) launch counts and mean us in a rocprofv3
--kernel-trace CSV of bench.py --profile (the timed region: after the last idle
gap of >= 40 ms, as prof_summary.py --after-gap) -- one kernel name serves
several row counts (n and 3n rows in the step), which prof_summary.py's
per-kernel table averages together.

usage: prof_by_grid.py TRACE.csv [NAME_REGEX] [--neighbours]
  default NAME_REGEX: the GAT backward source passes, the dX products with the
  GraphNorm-backward epilogue and the kernel that fuses the two
  --neighbours: a table row per (previous kernel -> next kernel) too: one kernel
  at one grid serves several places of the step (vg_gemm_chain's passes)
"""
import csv
import re
import sys

NEIGH = "--neighbours" in sys.argv
if NEIGH:
    sys.argv.remove("--neighbours")
PAT = sys.argv[2] if len(sys.argv) > 2 else \
    r"k_gat_bwd_src|k_gemm8w<false, 0, false, false, true|k_gemm16<false, 0, false, false, true"
from collections import defaultdict
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
gaps = [(int(rows[i + 1]["Start_Timestamp"]) - int(rows[i]["End_Timestamp"]), i) for i in range(len(rows) - 1)]
lg = [g for g in gaps if g[0] >= 40_000_000]
rows = rows[(lg[-1][1] if lg else max(gaps)[1]) + 1:]
gk = [k for k in rows[0] if "grid" in k.lower()]
wk = [k for k in rows[0] if "workgroup" in k.lower() and "size" in k.lower()]
tot = defaultdict(lambda: [0, 0.0])
def short_name(n):
    return re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "").replace("void ", ""))


for i, r in enumerate(rows):
    n = r["Kernel_Name"]
    if not re.search(PAT, n):
        continue
    short = short_name(n)
    if NEIGH:
        prev = re.sub(r"<.*", "", short_name(rows[i - 1]["Kernel_Name"])) if i else "-"
        nxt = re.sub(r"<.*", "", short_name(rows[i + 1]["Kernel_Name"])) if i + 1 < len(rows) else "-"
        short += f"  [{prev} -> {nxt}]"
    key = (short, "x".join(r[k] for k in gk), "x".join(r[k] for k in wk))
    tot[key][0] += 1
    tot[key][1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
for (n, g, w), (c, t) in sorted(tot.items()):
    print(f"{c:5d} x {t / c:8.2f} us  total {t / 1e3:7.3f} ms  grid {g} wg {w}  {n}")
