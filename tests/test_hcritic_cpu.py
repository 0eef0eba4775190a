"""The f16 critic scorer without a GPU: the host-only argument
checks of vg_hcritic_score and its two kernels' entry points, the arena query,
the Python refusals and the kernels' resource use (hipcc cross-compiles
gfx950)."""
from __future__ import annotations

import ctypes as ct
import os

import pytest
import torch

from parity_util import tiny_config
from test_critic_select_cpu import _usage
from vgan.config import Configuration

VG_EINVAL = -1
P = 256  # a non-NULL, 256-byte-aligned stand-in; never dereferenced on these paths
F, K, H = 29, 7, 64


def _model(h=H, classes=K, feat=F):
    """The default critic's description (64-64 MLP, 64-32-16-32-64 GAT, 64-32-16-8-1 decoder)."""
    from vgan._lib import VgHcriticModel

    md = VgHcriticModel()
    md.n_mlp, md.n_blocks, md.n_dec, md.has_sigmoid, md.classes = 2, 4, 4, 0, classes

    def lin(d, i, o, ldw=None):
        d.weight, d.ldw, d.weight_f32, d.bias, d.in_, d.out = P, (i + 7) // 8 * 8 if ldw is None else ldw, P, P, i, o

    lin(md.mlp[0], feat + classes, h, ldw=(feat + 7) // 8 * 8)
    lin(md.mlp[1], h, h)
    for b, (i, o) in enumerate(((h, h // 2), (h // 2, h // 4), (h // 4, h // 2), (h // 2, h))):
        d = md.block[b]
        d.lin_weight, d.ldw, d.att_src, d.att_dst, d.bias, d.slope = P, (i + 7) // 8 * 8, P, P, P, 0.2
        d.gn_weight = d.gn_bias = d.gn_mean_scale = P
        d.gn_eps, d.in_, d.out = 1e-5, i, o
    for j, (i, o) in enumerate(((h, h // 2), (h // 2, h // 4), (h // 4, h // 8), (h // 8, 1))):
        lin(md.dec[j], i, o)
    return md


def _batch(n=1000, copies=4, feat=F, graphs=4):
    from vgan._lib import VgHcriticBatch

    bt = VgHcriticBatch()
    bt.n, bt.copies, bt.feat, bt.num_edges, bt.num_graphs, bt.ld_mvx = n, copies, feat, 9 * n, graphs, (feat + 7) // 8 * 8
    bt.row_ptr = bt.col = bt.mvx = bt.pred = bt.ptr = P
    bt.copy_stride = n
    return bt


def _score(md, bt, arena=P, arena_bytes=None, scores=P, score=None, best=None, labels=None):
    from vgan._lib import LIB as lib

    if arena_bytes is None:
        arena_bytes = 1 << 40
    return lib.vg_hcritic_score(ct.byref(md), ct.byref(bt), arena, arena_bytes, scores, score, best, labels, None)


def _size(md, bt):
    from vgan._lib import LIB as lib

    return int(lib.vg_hcritic_arena_bytes(ct.byref(md), ct.byref(bt)))


def test_score_abi_checks_arguments_on_the_host():
    """Every refusal happens before any launch: the pointers are not device
    addresses (and no GPU is present here).  The last call of each group is
    the refusal; the description it departs from is accepted by the arena
    query."""
    from vgan._lib import LIB as lib

    assert _size(_model(), _batch()) > 0
    assert _score(_model(), _batch(n=0)) == VG_EINVAL and _size(_model(), _batch(n=0)) < 0
    assert _score(_model(), _batch(copies=0)) == VG_EINVAL and _size(_model(), _batch(copies=0)) < 0
    assert _score(_model(classes=33), _batch()) == VG_EINVAL and _size(_model(classes=33), _batch()) < 0  # K > 32
    assert _size(_model(classes=32), _batch()) > 0
    assert _score(_model(h=512), _batch()) == VG_EINVAL and _size(_model(h=512), _batch()) < 0  # H > 256
    bt = _batch()
    bt.ld_mvx = 36  # not a multiple of 8
    assert _score(_model(), bt) == VG_EINVAL and _size(_model(), bt) < 0
    md = _model()
    md.mlp[1].ldw = 68
    assert _score(md, _batch()) == VG_EINVAL
    md = _model()
    md.block[2].ldw = 20
    assert _score(md, _batch()) == VG_EINVAL
    assert _score(_model(), _batch(), scores=None) == VG_EINVAL
    assert _score(_model(), _batch(), arena=None) == VG_EINVAL
    assert _score(_model(), _batch(), arena=P + 16) == VG_EINVAL  # the arena's 256-byte alignment
    # the select tail: all three outputs or none
    for outs in ((P, None, None), (None, P, None), (None, None, P), (P, P, None), (P, None, P), (None, P, P)):
        assert _score(_model(), _batch(), score=outs[0], best=outs[1], labels=outs[2]) == VG_EINVAL, outs
    bt = _batch()
    bt.ptr = None
    assert _score(_model(), bt, score=P, best=P, labels=P) == VG_EINVAL  # the tail needs the buildings' rows
    assert _score(_model(), _batch(graphs=0), score=P, best=P, labels=P) == VG_EINVAL
    # an arena one byte short
    need = _size(_model(), _batch())
    assert _score(_model(), _batch(), arena_bytes=need - 1) == VG_EINVAL
    # widths that do not chain, a decoder that does not end in one score, NULL weights, rows that overlap
    md = _model()
    md.mlp[1].in_ = 48
    assert _score(md, _batch()) == VG_EINVAL and _size(md, _batch()) < 0
    md = _model()
    md.dec[3].out = 2
    assert _score(md, _batch()) == VG_EINVAL and _size(md, _batch()) < 0
    md = _model()
    md.block[1].out = 12  # rows of 16 halves hold 9..16 channels: fine
    md.block[2].in_ = 12
    assert _size(md, _batch()) > 0
    md.block[1].out = 20  # 24 halves: no aggregation kernel
    md.block[2].in_ = 20
    assert _score(md, _batch()) == VG_EINVAL and _size(md, _batch()) < 0
    md = _model()
    md.dec[2].weight_f32 = None
    assert _score(md, _batch()) == VG_EINVAL
    md = _model()
    md.block[0].att_src = None
    assert _score(md, _batch()) == VG_EINVAL
    bt = _batch()
    bt.copy_stride = bt.n - 1
    assert _score(_model(), bt) == VG_EINVAL
    bt = _batch()
    bt.pred = None
    assert _score(_model(), bt) == VG_EINVAL
    assert lib.vg_hcritic_arena_bytes(None, ct.byref(_batch())) == VG_EINVAL
    assert lib.vg_hcritic_score(None, ct.byref(_batch()), P, 1 << 40, P, None, None, None, None) == VG_EINVAL


def test_kernel_entry_points_check_arguments_on_the_host():
    from vgan._lib import LIB as lib

    def embed(base=P, ld_base=64, w=P, ldw=36, col0=29, classes=7, pred=P, stride=100, copies=3, n=100, h=64, y=P,
              ldy=64):
        return lib.vg_hcritic_embed_labels(base, ld_base, w, ldw, col0, classes, pred, stride, copies, n, h, y, ldy,
                                           None)

    assert embed(h=0, ld_base=0) == VG_EINVAL and embed(h=257, ld_base=257, ldy=264) == VG_EINVAL
    assert embed(classes=0) == VG_EINVAL and embed(classes=33, ldw=29 + 33) == VG_EINVAL
    assert embed(copies=0) == VG_EINVAL and embed(n=0, stride=0) == VG_EINVAL
    for name in ("base", "w", "pred", "y"):
        assert embed(**{name: None}) == VG_EINVAL
    assert embed(stride=99) == VG_EINVAL and embed(ld_base=63) == VG_EINVAL
    assert embed(ldw=35) == VG_EINVAL and embed(col0=-1) == VG_EINVAL
    assert embed(ldy=60) == VG_EINVAL and embed(ldy=56) == VG_EINVAL and embed(h=20, ld_base=20, ldy=20) == VG_EINVAL
    assert embed(y=P + 8) == VG_EINVAL  # 16-byte stores
    assert embed(copies=1 << 20, n=1 << 12, stride=1 << 12) == VG_EINVAL  # 2^32 stacked rows

    def decode(widths, x=P, ld=None, rows=10, nl=None, out=P, w=P):
        nl = len(widths) - 1 if nl is None else nl
        wd = (ct.c_int32 * len(widths))(*widths)
        ws = (ct.c_void_p * max(nl, 1))(*[w] * max(nl, 1))
        return lib.vg_hcritic_decode(x, widths[0] if ld is None else ld, rows, wd, nl, ws, ws, 0, out, None)

    assert decode([24, 12, 6, 3, 1]) == VG_EINVAL  # H = 24: the caller's per-layer path
    assert decode([256, 128, 64, 32, 1]) == VG_EINVAL and decode([8, 4, 2, 1, 1]) == VG_EINVAL
    assert decode([64, 32, 16, 8]) == VG_EINVAL and decode([64, 32, 16, 4, 1]) == VG_EINVAL
    assert decode([64, 32, 16, 8, 1], rows=0) == VG_EINVAL and decode([64, 32, 16, 8, 1], ld=60) == VG_EINVAL
    assert decode([64, 32, 16, 8, 1], x=None) == VG_EINVAL and decode([64, 32, 16, 8, 1], out=None) == VG_EINVAL
    assert decode([64, 32, 16, 8, 1], w=None) == VG_EINVAL
    assert lib.vg_hcritic_sigmoid(None, 5, None) == VG_EINVAL and lib.vg_hcritic_sigmoid(P, 0, None) == VG_EINVAL


def test_arena_grows_with_rows_and_copies():
    sizes_n = [_size(_model(), _batch(n=n)) for n in (1, 100, 1000, 1001, 12161)]
    assert all(s > 0 and s % 256 == 0 for s in sizes_n)
    assert all(a < b for a, b in zip(sizes_n, sizes_n[1:])), sizes_n
    sizes_k = [_size(_model(), _batch(copies=k)) for k in (1, 2, 3, 10, 17)]
    assert all(a < b for a, b in zip(sizes_k, sizes_k[1:])), sizes_k


def test_python_refusals():
    from vgan.half import HalfCritic
    from vgan.infer import InferenceSweep
    from vgan.models import VoxelGNNDiscriminator, VoxelGNNGenerator

    cfg = tiny_config(Configuration())
    cfg.DEVICE = "cpu"
    torch.manual_seed(0)
    G = VoxelGNNGenerator(cfg, 17, 12)
    D = VoxelGNNDiscriminator(cfg, 17, 12)
    with pytest.raises(ValueError, match="critic_dtype"):
        InferenceSweep(G, [1.0, 0.5], critic=D, critic_dtype="bf16")
    with pytest.raises(RuntimeError, match="ROCm device"):  # a CPU model: as HalfGenerator
        HalfCritic(D)
    with pytest.raises(RuntimeError, match="ROCm device"):
        InferenceSweep(G, [1.0, 0.5], critic=D, critic_dtype="f16")
    assert InferenceSweep(G, [1.0, 0.5], critic=D).half_critic is None  # f32 unless asked
    cfg2 = tiny_config(Configuration())
    cfg2.DEVICE = "cpu"
    cfg2.DISCRIMINATOR_CONV_TYPE = "GATV2CONV"
    D2 = VoxelGNNDiscriminator(cfg2, 17, 12)
    with pytest.raises(ValueError, match="GATCONV"):  # before anything touches a device
        HalfCritic(D2)
    with pytest.raises(ValueError, match="GATCONV"):
        InferenceSweep(G, [1.0, 0.5], critic=D2, critic_dtype="f16")
    assert InferenceSweep(G, [1.0, 0.5], critic=D2).D is D2  # the f32 path takes a GATv2 critic as before


def test_hcritic_kernels_spill_nothing_and_fit_lds():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    table = _usage("hcritic.hip")
    embed = {k: v for k, v in table.items() if "k_hcritic_embed_labels" in k}
    decode = {k: v for k, v in table.items() if "k_hcritic_decode" in k}
    assert len(embed) == 2 and len(decode) == 4, sorted(table)  # float4 / scalar base reads; H = 16, 32, 64, 128
    for name, u in sorted(table.items()):
        print(f"{name}: {u}")  # occupancy is recorded in DESIGN.md 4.54, not asserted
        assert u.get("spill", 0) == 0 and u.get("scratch", 0) == 0, (name, u)
    for name, u in embed.items():
        # static LDS; the label slab is dynamic: 32 classes x 256 columns x 4 bytes at the ABI's limits
        assert u["lds"] + 32 * 256 * 4 <= 32 * 1024, (name, u)
    for name, u in decode.items():
        assert u["lds"] <= 64 * 1024, (name, u)
