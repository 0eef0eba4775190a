"""vg_gat_bwd_gn_dx: the GAT backward source pass and the dX product it feeds
in one launch, against the unchanged two launches (vg_gat_bwd_gn, then
vg_gemm_gn_bwd on its g_h) on the same inputs.

Required: torch.equal on g_h (dH), dX, tpart, g_out and the whole backward
workspace (g_pre, g_a_dst and both partial sets, so the deferred att_src fold
sees the same rows), and on the folded parameter gradients.  The folded
g_att_src is also checked against an f64 sum formed on the CPU from the
reference path's inputs (g_pre of the workspace, h): the fused path's error
may be at most 2x the two-launch path's own error (plus one f32 ulp of the
column's absolute sum, for columns the reference happens to hit exactly).

Graphs are random (torch.randint edges plus self loops), built here so that
the CSC degrees the kernel branches on are all present: 0, exactly L, L + 1
(the non-shuffle path), more than 4 L, and degrees that are no multiple of 4.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

VG_EINVAL = -1
# C -> Cin of the default D and G encoders' blocks b > 0, plus a width that
# is no multiple of the 32-wide K-tile (zero-padded tail) or of the lane group
PAIRS = [(16, 8), (32, 16), (64, 32), (128, 64), (24, 12)]
# (segments, seg_rows, injections): a tail tile (N % 64 != 0), tiles that
# straddle a segment boundary (tpart slot 1), injections that start mid-tile
LAYOUTS = [(1, 64, False), (1, 257, False), (3, 64, False), (3, 100, True), (3, 257, True)]


def _lanes(c):  # lanes per row of the source pass (pick_fused_shape)
    return 8 if c <= 32 else 16


def _graph(n, lanes, gen, dev):
    """CSR (by destination) and CSC (by source) arrays of a random graph."""
    e0 = 3 * n
    src = torch.randint(0, n, (e0,), generator=gen)
    dst = torch.randint(0, n, (e0,), generator=gen)
    loops = torch.arange(n)
    src, dst = torch.cat([src, loops]), torch.cat([dst, loops])
    special = {3: 0, 5: lanes, 9: lanes + 1, 11: 4 * lanes + 3, 70 % n: 7}  # source node -> CSC degree
    keep = torch.ones(src.numel(), dtype=torch.bool)
    for node in special:
        keep &= src != node
    src, dst = src[keep], dst[keep]
    for node, deg in special.items():
        d = torch.randint(0, n, (deg,), generator=gen)
        src, dst = torch.cat([src, torch.full((deg,), node)]), torch.cat([dst, d])
    order = torch.sort(dst, stable=True).indices  # CSR order: slot k
    src, dst = src[order], dst[order]
    e = src.numel()
    row_ptr = torch.zeros(n + 1, dtype=torch.long)
    row_ptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    by_src = torch.sort(src, stable=True).indices
    csc_ptr = torch.zeros(n + 1, dtype=torch.long)
    csc_ptr[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
    deg = csc_ptr[1:] - csc_ptr[:-1]
    for node, want in special.items():
        assert int(deg[node]) == want
    i32 = lambda t: t.to(torch.int32).to(dev)
    return dict(n=n, e=e, row_ptr=i32(row_ptr), col=i32(src), csc_ptr=i32(csc_ptr), csc_slot=i32(by_src),
                csc_dst=i32(dst[by_src]), src=src)


def _case(dev, c, m, segs, seg_rows, inj, seed=0):
    gen = torch.Generator().manual_seed(1000 * c + 10 * seg_rows + segs + seed)
    n = segs * seg_rows
    g = _graph(n, _lanes(c), gen, dev)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)
    pos = lambda *s: (torch.rand(*s, generator=gen) + 0.5).to(dev)
    mask = lambda *s: (2.0 * (torch.rand(*s, generator=gen) < 0.5).float()).to(dev)
    inj_row0 = 2 * seg_rows if inj else 0
    t = dict(g=g, n=n, c=c, m=m, segs=segs, seg_rows=seg_rows, inj_row0=inj_row0,
             h=r(n, c), att_s=r(c), att_d=r(c), a_s=r(n), a_d=r(n), alpha=torch.rand(g["e"], generator=gen).to(dev),
             # the GraphNorm above the GATConv (vg_gn_bwd_in)
             x=r(n, c), keep=mask(n, c), g_y=r(n, c), w=r(c), b=r(c), ms=r(c),
             stats=torch.cat([r(segs, c), pos(segs, c)], 1).contiguous(), sums=r(segs, 2 * c),
             gn_inj=r(n - inj_row0, c) if inj else None, src_inj=r(n - inj_row0, c) if inj else None,
             # the product and the GraphNorm of the block below (vg_dx_in)
             W=r(c, m), x2=r(n, m), keep2=mask(n, m), w2=r(m), b2=r(m), ms2=r(m),
             stats2=torch.cat([r(segs, m), pos(segs, m)], 1).contiguous())
    return t


def _run(t, fused, pgrads, deferred=False):
    """One backward through the fused entry or the two launches -> (rc, outputs)."""
    from vgan._lib import LIB, VgDxIn, VgFold, VgGnBwdIn, ptr

    g, n, c, m, dev = t["g"], t["n"], t["c"], t["m"], t["h"].device
    st = torch.cuda.current_stream(dev).cuda_stream
    z = lambda *s: torch.zeros(*s, device=dev)
    out = dict(dO=z(n, c), dH=z(n, c), dX=z(n, m), tpart=z(int(LIB.vg_gemm_gn_tpart_floats(n, m))),
               ws=z(int(LIB.vg_gat_bwd_ws_floats(n, g["e"], c))), g_as=z(c), g_ad=z(c), g_b=z(c))
    gn = VgGnBwdIn(x=ptr(t["x"]), keep=ptr(t["keep"]), g_y=ptr(t["g_y"]), inj=ptr(t["gn_inj"]), weight=ptr(t["w"]),
                   bias=ptr(t["b"]), mean_scale=ptr(t["ms"]), stats=ptr(t["stats"]), sums=ptr(t["sums"]), eps=1e-5,
                   segments=t["segs"], seg_rows=t["seg_rows"], inj_offset=t["inj_row0"] * c if t["gn_inj"] is not None else 0)
    folds, nf = (VgFold * 3)(), ctypes.c_int32(0)
    pg = (ptr(out["g_as"]), ptr(out["g_ad"]), ptr(out["g_b"])) if pgrads else (None, None, None)
    args = (ptr(g["row_ptr"]), ptr(g["col"]), ptr(g["csc_ptr"]), ptr(g["csc_slot"]), ptr(g["csc_dst"]), n, g["e"], c,
            ptr(t["h"]), ptr(t["att_s"]), ptr(t["att_d"]), ptr(t["a_s"]), ptr(t["a_d"]), ptr(t["alpha"]),
            ctypes.byref(gn), ptr(out["dO"]), 0.2, ptr(out["dH"]), *pg, 0, ptr(t["src_inj"]), t["inj_row0"],
            ptr(out["ws"]), folds if deferred else None, ctypes.byref(nf) if deferred else None)
    gemm_args = (ptr(t["x2"]), ptr(t["keep2"]), t["seg_rows"], ptr(t["w2"]), ptr(t["b2"]), ptr(t["ms2"]), 1e-5,
                 ptr(t["stats2"]), ptr(out["tpart"]))
    if fused:
        dx = VgDxIn(B=ptr(t["W"]), ldb=m, M=m, C=ptr(out["dX"]), ldc=m, gn_x=gemm_args[0], keep=gemm_args[1],
                    seg_rows=gemm_args[2], weight=gemm_args[3], bias=gemm_args[4], mean_scale=gemm_args[5],
                    eps=gemm_args[6], stats=gemm_args[7], tpart=gemm_args[8])
        rc = LIB.vg_gat_bwd_gn_dx(*args, ctypes.byref(dx), st)
    else:
        rc = LIB.vg_gat_bwd_gn(*args, st)
        if rc == 0:
            rc = LIB.vg_gemm_gn_bwd(ptr(out["dH"]), c, ptr(t["W"]), m, n, m, c, ptr(out["dX"]), m, *gemm_args, st)
    if rc == 0 and deferred:
        assert nf.value == 3
        out["folds"] = [(f.width, f.k, f.ldo, f.accumulate, f.nsrc, f.src[0].rows, f.src[0].ld,
                         f.src[0].part - out["ws"].data_ptr()) for f in folds]
        rc = LIB.vg_fold_batch(folds, nf.value, st)
    torch.cuda.synchronize()
    return rc, out


def _assert_same(a, b):
    for k in ("dO", "dH", "dX", "tpart", "ws", "g_as", "g_ad", "g_b"):
        assert torch.equal(a[k], b[k]), k


def _att_src_f64(t, out):
    """g_att_src = sum_j gas_j h_j, gas_j = sum of g_pre over j's CSC edges, in f64 on the CPU."""
    g = t["g"]
    g_pre = out["ws"][: g["e"]].double().cpu()
    gas = torch.zeros(t["n"], dtype=torch.float64).index_add_(0, g["src"], g_pre)
    h = t["h"].double().cpu()
    return (gas[:, None] * h).sum(0), (gas[:, None] * h).abs().sum(0)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: "S%d_r%d%s" % (v[0], v[1], "_inj" if v[2] else ""))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda v: "%dto%d" % v)
def test_fused_matches_two_launches(cuda, pair, layout):
    c, m = pair
    segs, seg_rows, inj = layout
    t = _case(cuda, c, m, segs, seg_rows, inj)
    pgrads = (segs + seg_rows + c // 16) % 2 == 0 or inj  # requested and not requested, both over every pair
    rc_ref, ref = _run(t, False, pgrads)
    rc, got = _run(t, True, pgrads)
    assert rc_ref == 0 and rc == 0
    _assert_same(got, ref)
    assert ref["dX"].abs().sum() > 0 and ref["tpart"].abs().sum() > 0 and ref["dH"].abs().sum() > 0
    if pgrads:
        want, scale = _att_src_f64(t, ref)
        err_ref = (ref["g_as"].double().cpu() - want).abs()
        err = (got["g_as"].double().cpu() - want).abs()
        print("g_att_src |err| vs f64: two launches %.3e, fused %.3e" % (err_ref.max(), err.max()))
        assert bool((err <= 2.0 * err_ref + scale * 2.0 ** -23).all())


@pytest.mark.parametrize("pair", [(32, 16), (128, 64)], ids=lambda v: "%dto%d" % v)
def test_fused_deferred_folds_match(cuda, pair):
    """The engines' form: folds described for vg_fold_batch, accumulate into the gradients."""
    t = _case(cuda, pair[0], pair[1], 3, 100, True, seed=1)
    rc_ref, ref = _run(t, False, True, deferred=True)
    rc, got = _run(t, True, True, deferred=True)
    assert rc_ref == 0 and rc == 0
    assert got["folds"] == ref["folds"]
    _assert_same(got, ref)


def _refused(t):
    rc, got = _run(t, True, True)
    assert rc == VG_EINVAL
    for k in ("dO", "dH", "dX", "tpart", "ws"):  # refused before anything was launched
        assert not got[k].any(), k


@pytest.mark.parametrize("pair", [(8, 8), (18, 8), (256, 64), (128, 128)], ids=lambda v: "%dto%d" % v)
def test_shapes_without_a_fused_kernel_are_refused(cuda, pair):
    """C <= 8 (the edge-parallel pass), C no multiple of the lane vector, C > 128, M > 64: VG_EINVAL."""
    _refused(_case(cuda, pair[0], pair[1], 1, 64, False))


def test_rows_past_the_source_grid_cap_are_refused(cuda):
    """The two-launch source pass caps its grid at 4096 workgroups (32 rows each at
    L 8) and strides beyond it, which groups the att_src partials otherwise: refused."""
    _refused(_case(cuda, 16, 8, 1, 4096 * 32 + 64, False))


def test_many_tiles_loop_free(cuda):
    """Just under that cap: 2048 tiles, several workgroup rounds, every run of 32
    rows written to its own partial row (the inverse block remap over a large grid)."""
    t = _case(cuda, 16, 8, 1, 4096 * 32, False)
    rc_ref, ref = _run(t, False, True)
    rc, got = _run(t, True, True)
    assert rc_ref == 0 and rc == 0
    _assert_same(got, ref)


def knob_off_check():
    from vgan._lib import LIB

    for c, _ in PAIRS:
        for n in (64, 300, 13000, 39000):
            assert LIB.vg_bwd_src_gemm_use(n, c) == 0
    print("KNOB_OFF_OK")


def test_engines_take_the_fused_launch_where_it_is_resident(cuda):
    """vg_bwd_src_gemm_use, the engines' question: never for shapes without a kernel
    or for more tiles than one workgroup round holds."""
    from vgan._lib import LIB

    assert LIB.vg_bwd_src_gemm_use(13000, 8) == 0 and LIB.vg_bwd_src_gemm_use(13000, 18) == 0
    assert LIB.vg_bwd_src_gemm_use(13000, 256) == 0
    if not os.environ.get("VG_BWD_SRC_GEMM_SHAPES") and os.environ.get("VG_BWD_SRC_GEMM", "1") != "0":
        for c, _ in PAIRS:
            assert LIB.vg_bwd_src_gemm_use(64 * 4096, c) == 0
            # one tile per CU at most: resident on any device; C = 128 is left on two launches (unmeasured)
            assert LIB.vg_bwd_src_gemm_use(64 * 100, c) == (1 if c <= 64 else 0)


def test_knob_off_selects_the_two_launches(cuda):
    """VG_BWD_SRC_GEMM=0 (read once, so in a process of its own): the engines are
    told to make the two launches, vg_gat_bwd_gn + vg_gemm_gn_bwd, at every shape."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import conftest, test_bwd_src_gemm_gpu as t; t.knob_off_check()" % here
    env = dict(os.environ, VG_BWD_SRC_GEMM="0")
    env.pop("VG_BWD_SRC_GEMM_SHAPES", None)
    proc = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0 and "KNOB_OFF_OK" in proc.stdout, proc.stdout + proc.stderr
