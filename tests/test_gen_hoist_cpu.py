"""vg_gen_hoist_arena_floats runs the hoisted pair of calls
(vg_gen_forward_stacked + vg_gen_loss_and_grad_from) dry -- no launch, no
device pointer read -- so its gating is testable without a GPU: a host-only
addition to the GPU tests of tests/test_gen_hoist_gpu.py, which cannot reach
the row counts at which the aggregation changes its kernel form."""
import ctypes as ct

from vgan._lib import LIB as lib, VgGenBatch, VgGenModel, VgGenStack

K, FL, VD, ZD, H, F = 7, 17, 12, 128, 128, 29


BLOCKS = ((H, 64), (64, 2), (2, 1), (1, 8))
BLOCKS_128 = ((H, 128), (128, 64), (64, 2), (2, 8))  # a 128-channel block, as the generator's first


def _model(first_out=128, blocks=BLOCKS):
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
    ln(md.dec[0], 8 + H + H + VD + ZD, 128)
    ln(md.dec[1], 128, 16)
    md.dec_last.in_, md.dec_last.out = 16, K
    md.dmlp[0].in_, md.dmlp[0].out = F + K, 64
    md.dmlp[1].in_, md.dmlp[1].out = 64, 64
    blk(md.dblock[0], 64, 32)
    blk(md.dblock[1], 32, 16)
    md.ddec[0].in_, md.ddec[0].out = 16, 8
    md.ddec[1].in_, md.ddec[1].out = 8, 1
    return md


def _size(md, n, copies, stacked_nodes=None, bf16=0):
    bt = VgGenBatch()
    bt.n, bt.classes, bt.mx_w, bt.vx_w, bt.mvx_w, bt.z_dim = n, K, FL, VD, F, ZD
    bt.num_graphs, bt.seg_rows = 4, n
    bt.g.num_nodes, bt.g.num_edges = n, 9 * n
    sk = VgGenStack()
    sk.copies, sk.iter_delta = copies, copies + 1
    sk.gs.num_nodes = (copies + 1) * n if stacked_nodes is None else stacked_nodes
    sk.gs.num_edges = (copies + 1) * 9 * n
    md.bf16 = bf16
    whole = int(lib.vg_gen_arena_floats(ct.byref(md), ct.byref(bt)))
    return whole, int(lib.vg_gen_hoist_arena_floats(ct.byref(md), ct.byref(bt), ct.byref(sk)))


def test_hoisted_arena_holds_the_stacked_forward_and_the_rest():
    md = _model()
    whole, hoisted = _size(md, 1880, 5)
    assert whole > 0 and hoisted > whole and hoisted % 64 == 0
    assert _size(md, 1880, 10)[1] > hoisted
    assert lib.vg_gen_state_bytes() > 0


def test_hoist_refuses_what_it_was_not_built_for():
    md = _model()
    assert _size(md, 1880, 0)[1] < 0                       # no label copy
    assert _size(md, 1880, 5, stacked_nodes=5 * 1880)[1] < 0  # a graph stacked another number of times
    assert _size(md, 1880, 5, bf16=1)[1] < 0               # f32 only
    # a first layer outside (64, 128] has no multi-source kernel
    assert _size(_model(first_out=64), 1880, 5)[1] < 0
    VG_EINVAL = -1
    bt, sk = VgGenBatch(), VgGenStack()
    assert lib.vg_gen_forward_stacked(ct.byref(md), ct.byref(bt), ct.byref(sk), None, 0, None, None, None,
                                      None) == VG_EINVAL
    assert lib.vg_gen_loss_and_grad_from(ct.byref(md), ct.byref(bt), None, None, 0, None, None) == VG_EINVAL


def test_hoist_refuses_a_slice_form_that_switches_on_between_the_row_counts():
    """The 64-channel slice form of the aggregation (C = 128, from
    VG_FWD_SLICE_ROWS = 100,000 rows) has the partial-block rows of the plain
    form, so vg_gat_gnp_rows cannot tell them apart: the gate asks
    vg_gat_fwd_sliced.  Sliced at 6 n but not at n (n = 17,000), or at 5 n and
    6 n but not at n (n = 20,001): refused.  Below the threshold at all three
    (n = 16,000): taken.  Without a 128-channel block nothing slices."""
    assert [lib.vg_gat_fwd_sliced(r, 128) for r in (17_000, 85_000, 99_999, 100_000, 102_000)] == [0, 0, 0, 1, 1]
    assert [lib.vg_gat_fwd_sliced(102_000, c) for c in (1, 8, 64, 96, 128, 192, 256)] == [0, 0, 0, 0, 1, 1, 1]
    assert lib.vg_gat_gnp_rows(17_000, 128) == lib.vg_gat_gnp_rows(102_000, 128)  # why gnp_rows is no gate here
    wide = _model(blocks=BLOCKS_128)
    assert _size(wide, 16_000, 5)[1] > 0
    assert _size(wide, 17_000, 5)[1] < 0
    assert _size(wide, 20_001, 5)[1] < 0
    assert _size(wide, 17_000, 5)[0] > 0  # the whole iteration at n rows is unaffected
    assert _size(_model(), 17_000, 5)[1] > 0
