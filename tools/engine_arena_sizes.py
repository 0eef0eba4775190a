"""The arena sizes the C++ engines' dry schedules report (vg_gen_arena_floats,
vg_gen_hoist_arena_floats, vg_critic_arena_floats) over a table of models,
row counts, copy counts and precisions, refused cases included.  No GPU.

    python tools/engine_arena_sizes.py                # this tree's library
    python tools/engine_arena_sizes.py OTHER_LIB.so   # beside another build's

A host-only restructuring of csrc/*_engine.hip must leave every value as it
was: the sizes are the sum of the schedule's `take`s
(profiles/engine_split_arena_sizes.txt)."""
import ctypes as ct
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "building-gan-graph-conditioned-architectural-volume-generation_amd"))
from vgan._lib import LIB, VgCriticBatch, VgCriticModel, VgGenBatch, VgGenModel, VgGenStack  # noqa: E402

K, FL, VD, ZD, H, F = 7, 17, 12, 128, 128, 29
BLOCKS = ((H, 64), (64, 2), (2, 1), (1, 8))            # tests/test_gen_hoist_cpu.py
BLOCKS_128 = ((H, 128), (128, 64), (64, 2), (2, 8))
NS = (64, 1000, 1880, 14488, 16000, 17000, 20001)
FNS = ("vg_gen_arena_floats", "vg_gen_hoist_arena_floats", "vg_critic_arena_floats")


def gen_model(blocks, first_out=128, dec_w=128, dec_in=None):
    md = VgGenModel()
    md.n_mfe, md.n_mlp, md.n_gblocks, md.n_dec = 2, 2, 4, 2
    md.n_dmlp, md.n_dblocks, md.n_ddec = 2, 2, 2
    md.tau, md.p_drop_g, md.p_drop_d = 1.0, 0.2, 0.2

    def ln(d, i, o):
        d.in_, d.out, d.ln_eps, d.slope = i, o, 1e-5, 0.2

    def blk(d, i, o):
        d.in_, d.out, d.gn_eps, d.slope = i, o, 1e-5, 0.2

    ln(md.mfe[0], FL, H)
    ln(md.mfe[1], H, H)
    ln(md.mlp[0], H + VD + ZD, first_out)
    ln(md.mlp[1], first_out, H)
    for b, (i, o) in enumerate(blocks):
        blk(md.gblock[b], i, o)
    ln(md.dec[0], blocks[-1][1] + H + H + VD + ZD if dec_in is None else dec_in, dec_w)
    ln(md.dec[1], dec_w, 16)
    md.dec_last.in_, md.dec_last.out = 16, K
    md.dmlp[0].in_, md.dmlp[0].out = F + K, 64
    md.dmlp[1].in_, md.dmlp[1].out = 64, 64
    blk(md.dblock[0], 64, 32)
    blk(md.dblock[1], 32, 16)
    md.ddec[0].in_, md.ddec[0].out = 16, 8
    md.ddec[1].in_, md.ddec[1].out = 8, 1
    return md


def critic_model(dec=(32, 16, 8, 1)):
    """The reference discriminator's pattern (models.py:162-279): MLP 64-64,
    GAT blocks 64-64-64, decoder 64-32-16-8-1."""
    md = VgCriticModel()
    md.n_mlp, md.n_blocks, md.n_dec = 2, 3, len(dec)
    md.lambda_gp, md.p_drop = 10.0, 0.2
    w = F + K
    for i in range(2):
        md.mlp[i].in_, md.mlp[i].out = w, 64
        w = 64
    for b in range(3):
        d = md.block[b]
        d.in_, d.out, d.gn_eps, d.slope = w, 64, 1e-5, 0.2
    for i, o in enumerate(dec):
        md.dec[i].in_, md.dec[i].out = w, o
        w = o
    return md


def gen_sizes(lib, md, n, copies, bf16=0, stacked_nodes=None, seg_rows=None):
    bt = VgGenBatch()
    bt.n, bt.classes, bt.mx_w, bt.vx_w, bt.mvx_w, bt.z_dim = n, K, FL, VD, F, ZD
    bt.num_graphs, bt.seg_rows = 4, n if seg_rows is None else seg_rows
    bt.g.num_nodes, bt.g.num_edges = n, 9 * n
    sk = VgGenStack()
    sk.copies, sk.iter_delta = copies, copies + 1
    sk.gs.num_nodes = (copies + 1) * n if stacked_nodes is None else stacked_nodes
    sk.gs.num_edges = (copies + 1) * 9 * n
    md.bf16 = bf16
    return (int(lib.vg_gen_arena_floats(ct.byref(md), ct.byref(bt))),
            int(lib.vg_gen_hoist_arena_floats(ct.byref(md), ct.byref(bt), ct.byref(sk))))


def critic_size(lib, md, n, bf16=0, g3_nodes=None):
    bt = VgCriticBatch()
    bt.n, bt.feat, bt.classes = n, F, K
    bt.g1.num_nodes, bt.g1.num_edges = n, 9 * n
    bt.g3.num_nodes, bt.g3.num_edges = 3 * n if g3_nodes is None else g3_nodes, 27 * n
    md.bf16 = bf16
    return int(lib.vg_critic_arena_floats(ct.byref(md), ct.byref(bt)))


def table(lib):
    rows = []
    models = (("blocks", gen_model(BLOCKS)), ("blocks128", gen_model(BLOCKS_128)),
              ("abi", gen_model(BLOCKS, first_out=H, dec_w=64)))  # tests/test_abi_cpu.py's
    for name, md in models:
        for n in NS:
            for copies in (1, 5, 10):
                for bf16 in (0, 1):
                    whole, hoist = gen_sizes(lib, md, n, copies, bf16)
                    rows.append((f"gen {name} n={n} copies={copies} bf16={bf16} whole", whole))
                    rows.append((f"gen {name} n={n} copies={copies} bf16={bf16} hoist", hoist))
    refused = (("first_out=64", gen_model(BLOCKS, first_out=64), {}),
               ("copies=0", gen_model(BLOCKS), {"copies": 0}),
               ("stacked_nodes=5n", gen_model(BLOCKS), {"stacked_nodes": 5 * 1880}),
               ("seg_rows=n/2", gen_model(BLOCKS), {"seg_rows": 940}),
               ("n=32", gen_model(BLOCKS), {"n": 32}),
               ("dec0.in=wrong", gen_model(BLOCKS, dec_in=H + H + VD + ZD), {}))
    for name, md, kw in refused:
        args = {"n": 1880, "copies": 5, **kw}
        whole, hoist = gen_sizes(lib, md, **args)
        rows.append((f"gen refused {name} whole", whole))
        rows.append((f"gen refused {name} hoist", hoist))
    for name, md in (("ref", critic_model()), ("dec8-1", critic_model(dec=(8, 1)))):
        for n in NS:
            for bf16 in (0, 1):
                rows.append((f"critic {name} n={n} bf16={bf16}", critic_size(lib, md, n, bf16)))
    rows.append(("critic refused n=32", critic_size(lib, critic_model(), 32)))
    rows.append(("critic refused g3=2n", critic_size(lib, critic_model(), 1880, g3_nodes=2 * 1880)))
    rows.append(("critic refused dec ends at 8", critic_size(lib, critic_model(dec=(32, 16, 8)), 1880)))
    return rows


def main():
    libs = [LIB]
    if len(sys.argv) > 1:
        other = ct.CDLL(sys.argv[1])
        for fn in FNS:
            getattr(other, fn).restype = ct.c_int64
        libs.append(other)
    cols = [table(lib) for lib in libs]
    print("# case | this tree" + (" | " + os.path.basename(sys.argv[1]) if len(libs) > 1 else ""))
    differ = 0
    for i, (case, v) in enumerate(cols[0]):
        vals = [c[i][1] for c in cols]
        differ += len(set(vals)) > 1
        print(case + " | " + " | ".join(str(x) for x in vals))
    if len(libs) > 1:
        print(f"# {len(cols[0])} cases, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
