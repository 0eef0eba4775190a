"""Launch the GATv2 kernels and GATConv's at the same shapes, for a kernel trace.

usage: python tools/gatv2_probe.py [--reps R]      (under tools/gatv2_trace.sh)

The batch is bench.py's first pooled one (32 synthetic buildings, N ~ 12.6k
rows, ~9 edges a row).  For C in (16, 64, 128): R launches each of
vg_gatv2_fwd / vg_gatv2_bwd (x_l, x_r the halves of one [N, 2C] buffer, as the
model passes them) and of vg_gat_aggregate_fwd / vg_gat_bwd_ex.  Prints one
JSON line with the bytes every launch must move (compulsory traffic: each
distinct row of an operand once, the edge arrays once), so durations from the
trace turn into rates against the 8 TB/s roofline.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "building-gan-graph-conditioned-architectural-volume-generation_amd"))

from vgan import ops  # noqa: E402
from vgan._lib import LIB, check, ptr  # noqa: E402
from vgan.graph import GraphBatch  # noqa: E402
from vgan.synth import SyntheticDataset  # noqa: E402


def must_move(n: int, e: int, c: int) -> dict:
    """Bytes per launch (f32 / int32 = 4 bytes)."""
    row, idx = 4 * n * c, 4 * (n + 1)
    return {
        # x_l rows + x_r rows + out, row_ptr + col, alpha
        "gatv2_fwd": 3 * row + idx + 4 * e + 4 * e,
        # x_l, x_r, g_out read, g_xr written; row_ptr + col, alpha read, ge written
        "gatv2_bwd_rows": 4 * row + idx + 4 * e + 8 * e,
        # x_l, x_r, g_out read, g_xl written; csc_ptr + slot + dst, alpha + ge read
        "gatv2_bwd_src": 4 * row + idx + 8 * e + 8 * e,
        # h + out, a_src + a_dst, row_ptr + col, alpha
        "gat_aggregate_fwd": 2 * row + 8 * n + idx + 4 * e + 4 * e,
        # h, g_out read; a_src, a_dst read, g_a_dst written; row_ptr + col, alpha read, g_pre written
        "gat_bwd_rows": 2 * row + 12 * n + idx + 4 * e + 8 * e,
        # h, g_out read, g_h written; g_a_dst; csc arrays, alpha + g_pre read
        "gat_bwd_src": 3 * row + 4 * n + idx + 8 * e + 8 * e,
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ds = SyntheticDataset(6500, seed=777)
    vox = GraphBatch.from_data_list([ds[i][1] for i in range(32)])
    n = vox.num_nodes
    csr = ops.CSR(vox.edge_index.to(dev), n)
    e = csr.num_edges
    st = csr.stream()
    out = {"rows": n, "edges": e, "reps": args.reps, "bytes": {}}
    torch.manual_seed(0)
    for c in (16, 64, 128):
        y = torch.randn(n, 2 * c, device=dev)
        x_l, x_r = y[:, :c], y[:, c:]
        att, bias = torch.randn(c, device=dev) / c ** 0.5, torch.randn(c, device=dev)
        g_out = torch.randn(n, c, device=dev)
        o, alpha = torch.empty(n, c, device=dev), torch.empty(e, device=dev)
        g_y, g_att, g_bias = torch.empty(n, 2 * c, device=dev), torch.empty(c, device=dev), torch.empty(c, device=dev)
        ws = torch.empty(int(LIB.vg_gatv2_bwd_ws_floats(n, e, c)), device=dev)
        h = x_l.contiguous()
        att_d = torch.randn(c, device=dev) / c ** 0.5
        a_s, a_d = h @ att, h @ att_d
        g_h, g_vs, g_vd = torch.empty(n, c, device=dev), torch.empty(c, device=dev), torch.empty(c, device=dev)
        ws1 = torch.empty(int(LIB.vg_gat_bwd_ws_floats(n, e, c)), device=dev)
        for _ in range(args.reps):
            check(LIB.vg_gatv2_fwd(ptr(csr.row_ptr), ptr(csr.col), n, c, ptr(x_l), 2 * c, ptr(x_r), 2 * c, ptr(att),
                                   ptr(bias), 0.2, ptr(o), ptr(alpha), st), "vg_gatv2_fwd")
            check(LIB.vg_gatv2_bwd(ptr(csr.row_ptr), ptr(csr.col), ptr(csr.csc_ptr), ptr(csr.csc_slot),
                                   ptr(csr.csc_dst), n, e, c, ptr(x_l), 2 * c, ptr(x_r), 2 * c, ptr(att), ptr(alpha),
                                   ptr(g_out), 0.2, ptr(g_y[:, :c]), 2 * c, ptr(g_y[:, c:]), 2 * c, ptr(g_att),
                                   ptr(g_bias), 0, ptr(ws), st), "vg_gatv2_bwd")
        for _ in range(args.reps):
            check(LIB.vg_gat_aggregate_fwd(ptr(csr.row_ptr), ptr(csr.col), n, c, ptr(h), ptr(a_s), ptr(a_d),
                                           ptr(bias), 0.2, ptr(o), ptr(alpha), st), "vg_gat_aggregate_fwd")
            check(LIB.vg_gat_bwd_ex(ptr(csr.row_ptr), ptr(csr.col), ptr(csr.csc_ptr), ptr(csr.csc_slot),
                                    ptr(csr.csc_dst), n, e, c, ptr(h), ptr(att), ptr(att_d), ptr(a_s), ptr(a_d),
                                    ptr(alpha), ptr(g_out), 0.2, ptr(g_h), ptr(g_vs), ptr(g_vd), ptr(g_bias), 0, None,
                                    0, ptr(ws1), st), "vg_gat_bwd_ex")
        out["bytes"][c] = must_move(n, e, c)
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
