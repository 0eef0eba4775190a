"""vg_gemm_chain: the discriminator's MLP encoder with the block-0 projection,
and its adjoint and tangent runs, as one launch per pass -- against the
separate launches (vg_gemm per layer, vg_gat_lin_att) on the same inputs.

Required: every stored output, a_src / a_dst included, has the bits of the
separate launches' (compared as int32, so the NaN the outputs are pre-filled
with compares too), and nothing is written outside the rows and columns asked
for.  The operands are laid out as the engines lay them out: row-offset views
of taller buffers (the mix rows at 2n as mask sources, the tangent rows at 3n
as outputs of the same buffer), the `weight + F` column window of the first
layer with ldw = W0, and, in the padded cases, row strides above the widths.

The engines: the critic and the generator iteration with the chain on and off
(the knob is read once, so the other setting runs in a process of its own)
give bit-identical losses and flat gradients, and the chained entry point is
the one taken (vg_gemm_chain_launches)."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

VG_EINVAL = -1
W0, HD = 36, 64  # the first layer's input width, the MLP's width
# (mvx features F, classes): 12 classes on an aligned window, and the models' own 29 + 7, whose `weight + F`
# window allows no 16-byte loads and whose label tangent has K = 7 (refused: that product stays a launch of its own)
SPLITS = [(24, 12), (29, 7)]
ROWS = [1, 63, 64, 65, 129, 3 * 257]
KINDS = ["passA", "passB_tail", "passC_head", "passD_tail", "gen_tail"]


def _ptr(t, off=0):
    return t.data_ptr() + 4 * off


def _case(kind, r, c0, pad, dev, F=24, KC=12):
    """Operands of one chain over r rows, deterministic.  A link: w (tensor,
    float offset), ldw, trans, m, bias, act, aux / out (tensor, first row),
    att.  Returns (x tensor, float offset, ldx, k, links)."""
    g = torch.Generator().manual_seed(100 * r + c0 + pad)

    def rnd(*s, scale=1.0):
        return (torch.randn(*s, generator=g) * scale).to(dev)

    def tall(rows_random, rows_total, width):  # random rows, then NaN rows the chain may fill
        t = torch.full((rows_total, width), float("nan"), device=dev)
        t[:rows_random] = rnd(rows_random, width)
        return t

    Wa, ba = rnd(HD, W0, scale=0.3), rnd(HD)
    Wb, bb = rnd(HD, HD, scale=0.2), rnd(HD)
    Wl, ats, atd = rnd(c0, HD, scale=0.2), rnd(c0), rnd(c0)
    ld = HD + pad
    mrow, trow = 2 * r, 3 * r
    att = lambda H, a_s, a_d: dict(w=(Wl, 0), ldw=HD, trans=0, m=c0, bias=None, act=0, aux=None, out=(H, 0), ld=c0,
                                   att=(ats, atd, a_s, a_d))
    lin = lambda w, ldw, trans, m, bias, act, aux, out, ld_: dict(w=w, ldw=ldw, trans=trans, m=m, bias=bias, act=act,
                                                                  aux=aux, out=out, ld=ld_, att=None)
    if kind == "passA":  # X0 -> mlp[0] -> mlp[1] -> block-0 projection, all rows
        X0 = tall(r, r + 3, W0 + pad)
        m0, m1 = tall(0, r + 3, ld), tall(0, r + 3, ld)
        H, a_s, a_d = tall(0, r + 3, c0), tall(0, r + 3, 1), tall(0, r + 3, 1)
        links = [lin((Wa, 0), W0, 0, HD, ba, 1, None, (m0, 0), ld), lin((Wb, 0), HD, 0, HD, bb, 1, None, (m1, 0), ld),
                 att(H, a_s, a_d)]
        if pad:  # the projection's H is written with ld = C: its operand must be contiguous
            links = links[:2]
        return X0, 0, W0 + pad, W0, links
    if kind in ("passB_tail", "gen_tail"):  # dH -> masked dX -> mlp[1] adjoint -> the label columns' adjoint
        off = trow if kind == "passB_tail" else 0
        aoff = mrow if kind == "passB_tail" else 0
        total = 4 * r if kind == "passB_tail" else r + 3
        dH = tall(off + r, off + r + 3, c0)
        m0, m1 = tall(aoff + r, total, ld), tall(aoff + r, total, ld)
        a0, a1 = tall(0, total, ld), tall(0, total, ld)
        gl = tall(0, r + 3, KC + pad)
        last = lin((Wa, F), W0, 1, KC, None, 0, None, (gl, 0), KC + pad)
        if kind == "gen_tail":  # the loss head's adjoint summed in (act 4)
            gh = tall(r, r + 3, KC + pad)
            last = lin((Wa, F), W0, 1, KC, None, 4, (gh, 0), (gl, 0), KC + pad)
        links = [lin((Wl, 0), HD, 1, HD, None, 3, (m1, aoff), (a1, off), ld),
                 lin((Wb, 0), HD, 1, HD, None, 3, (m0, aoff), (a0, off), ld), last]
        return dH, off * c0, c0, c0, links
    if kind == "passC_head":  # u0 (X0's label columns, tangent rows) -> tangents -> block-0 tangent projection
        X0 = tall(4 * r, 4 * r, W0)
        m0, m1 = tall(trow, 4 * r, ld), tall(trow, 4 * r, ld)  # mask from the mix rows, tangent rows written
        H, a_s, a_d = tall(0, r + 3, c0), tall(0, r + 3, 1), tall(0, r + 3, 1)
        links = [lin((Wa, F), W0, 0, HD, None, 3, (m0, mrow), (m0, trow), ld),
                 lin((Wb, 0), HD, 0, HD, None, 3, (m1, mrow), (m1, trow), ld), att(H, a_s, a_d)]
        if pad:
            links = links[:2]
        return X0, trow * W0 + F, W0, KC, links
    assert kind == "passD_tail"  # dH -> masked dX -> mlp[1] adjoint, all rows
    dH = tall(r, r + 3, c0)
    m0, m1 = tall(r, r + 3, ld), tall(r, r + 3, ld)
    a0, a1 = tall(0, r + 3, ld), tall(0, r + 3, ld)
    links = [lin((Wl, 0), HD, 1, HD, None, 3, (m1, 0), (a1, 0), ld), lin((Wb, 0), HD, 1, HD, None, 3, (m0, 0), (a0, 0), ld)]
    return dH, 0, c0, c0, links


def _at(pair, ld):
    return _ptr(pair[0], pair[1] * ld) if pair is not None else None


def _separate(xp, ldx, k, links, r):
    from vgan._lib import LIB

    for L in links:
        out = _at(L["out"], L["ld"])
        if L["att"]:
            ats, atd, a_s, a_d = L["att"]
            rc = LIB.vg_gat_lin_att(xp, ldx, _ptr(*L["w"]), r, k, L["m"], _ptr(ats), _ptr(atd), out, _ptr(a_s), _ptr(a_d),
                                    None)
        else:
            rc = LIB.vg_gemm(xp, ldx, _ptr(*L["w"]), L["ldw"], 0 if L["trans"] else 1,
                             _ptr(L["bias"]) if L["bias"] is not None else None, L["act"], _at(L["aux"], L["ld"]), L["ld"],
                             out, L["ld"], r, L["m"], k, None)
        assert rc == 0
        xp, ldx, k = out, L["ld"], L["m"]
    return xp, ldx, k


def _chain(xp, ldx, k, links, r, bf16=0):
    from vgan._lib import LIB, VgGemmLink

    arr = (VgGemmLink * len(links))()
    for a, L in zip(arr, links):
        a.w, a.ldw, a.w_trans, a.m, a.act = _ptr(*L["w"]), L["ldw"], L["trans"], L["m"], L["act"]
        a.bias = _ptr(L["bias"]) if L["bias"] is not None else None
        a.aux, a.ld_aux = _at(L["aux"], L["ld"]), L["ld"] if L["aux"] is not None else 0
        a.out, a.ld_out = _at(L["out"], L["ld"]), L["ld"]
        if L["att"]:
            a.att_src, a.att_dst, a.a_src, a.a_dst = (_ptr(t) for t in L["att"])
    return LIB.vg_gemm_chain(xp, ldx, k, r, arr, len(links), bf16, None)


def _as_the_engines(xp, ldx, k, links, r):
    """Ctx::links_or_gemms: the links from i on as a chain; where that is refused, link i alone and the rest again.
    Returns the refusals."""
    refused = 0
    for i in range(len(links) - 1):
        rc = _chain(xp, ldx, k, links[i:], r)
        if rc == 0:
            return refused
        assert rc == VG_EINVAL
        refused += 1
        xp, ldx, k = _separate(xp, ldx, k, links[i:i + 1], r)
    _separate(xp, ldx, k, links[-1:], r)  # one link left: no chain
    return refused


def _bits(t):
    return t.view(torch.int32)


def _written(links, r):
    """{id(buffer): (buffer, mask of the elements the chain may write)}"""
    res = {}
    for L in links:
        outs = [(L["out"][0], L["out"][1], L["m"])]
        if L["att"]:
            outs += [(L["att"][2], 0, 1), (L["att"][3], 0, 1)]
        for t, row0, m in outs:
            _, mask = res.setdefault(id(t), (t, torch.zeros_like(t, dtype=torch.bool)))
            mask[row0:row0 + r, :m] = True
    return res


@pytest.mark.parametrize("pad", [0, 4], ids=["ld=width", "ld>width"])
@pytest.mark.parametrize("split", SPLITS, ids=lambda v: "F%d+%d" % v)
@pytest.mark.parametrize("kind", KINDS)
def test_chain_has_the_bits_of_the_separate_launches(cuda, kind, split, pad):
    for r in ROWS:
        for c0 in (64, 32):
            x, xoff, ldx, k, links = _case(kind, r, c0, pad, cuda, *split)
            outs = [t for t, _ in _written(links, r).values()]
            before = [t.clone() for t in outs]
            _separate(_ptr(x, xoff), ldx, k, links, r)
            torch.cuda.synchronize()
            ref = outs
            x, xoff, ldx, k, links = _case(kind, r, c0, pad, cuda, *split)
            masks = _written(links, r)
            outs = [t for t, _ in masks.values()]
            calls = _launches()
            # only the label columns' tangent with K = 7 is refused: one launch of its own, then the chain
            refused = _as_the_engines(_ptr(x, xoff), ldx, k, links, r)
            assert refused == (kind == "passC_head" and split[1] % 4 != 0)
            torch.cuda.synchronize()
            assert _launches() == calls + (1 if len(links) - refused >= 2 else 0)
            for got, want in zip(outs, ref):
                assert torch.equal(_bits(got), _bits(want)), (kind, r, c0)
            for got, was in zip(outs, before):
                t, mask = masks[id(got)]
                assert bool(torch.isfinite(got[mask]).all()) and bool(mask.any()), (kind, r, c0)
                assert bool(((_bits(got) == _bits(was)) | mask).all()), (kind, r, c0)  # nothing else written


def _launches():
    from vgan._lib import LIB

    return int(LIB.vg_gemm_chain_launches())


@pytest.mark.parametrize("what", ["width 68", "k 10", "bf16"])
def test_shapes_without_a_chain_kernel_are_refused(cuda, what):
    """A width above 64, a K that is no multiple of 4 (the per-layer path loads
    such operands as scalars), bf16: VG_EINVAL before anything is launched."""
    r = 129
    g = torch.Generator().manual_seed(5)
    nan = lambda *s: torch.full(s, float("nan"), device=cuda)
    m, k = (68, 64) if what == "width 68" else (64, 10) if what == "k 10" else (64, 64)
    x = torch.randn(r, 64, generator=g).to(cuda)
    W1, W2 = torch.randn(m, 64, generator=g).to(cuda), torch.randn(64, 72, generator=g).to(cuda)
    o1, o2 = nan(r, 72), nan(r, 64)
    lin = lambda w, ldw, m_, out, ld: dict(w=(w, 0), ldw=ldw, trans=0, m=m_, bias=None, act=0, aux=None, out=(out, 0),
                                           ld=ld, att=None)
    links = [lin(W1, 64, m, o1, 72), lin(W2, 72, 64, o2, 64)]
    calls = _launches()
    assert _chain(_ptr(x), 64, k, links, r, bf16=1 if what == "bf16" else 0) == VG_EINVAL
    torch.cuda.synchronize()
    assert _launches() == calls
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2).all())
    if what == "bf16":  # the same links are taken in f32
        assert _chain(_ptr(x), 64, k, links, r) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o1[:, :64]).all()) and bool(torch.isfinite(o2).all())


def engine_outputs(path=None):
    """One critic iteration and one generator iteration of the native engines on
    4 synthetic buildings: losses, flat gradients, chains launched."""
    from vgan.config import Configuration
    from vgan.models import VoxelGNNDiscriminator, VoxelGNNGenerator
    from vgan.synth import SyntheticDataset
    from vgan.trainer import Trainer

    dev = "cuda:0"
    cfg = Configuration()
    cfg.DEVICE = dev
    cfg.runtime["rng"] = "device"
    cfg.runtime["precision"] = "f32"
    cfg.runtime["gen"] = "engine"
    torch.manual_seed(cfg.SEED)
    G, D = VoxelGNNGenerator(cfg, 17, 12), VoxelGNNDiscriminator(cfg, 17, 12)
    tr = Trainer(G, D, None, torch.optim.Adam(G.parameters(), lr=2e-4, betas=cfg.BETAS),
                 torch.optim.Adam(D.parameters(), lr=2e-4, betas=cfg.BETAS), None, cfg)
    loc, vox = SyntheticDataset(4, seed=99).batch(range(4))
    loc, vox = loc.to(dev), vox.to(dev)
    assert vox.x.shape[0] >= 64
    with torch.no_grad():
        _, hard, soft = tr._generate(loc, vox)
    hard, soft = hard.clone(), soft.clone()
    tr.flat_d.grad.zero_()
    tr.rng.reset()
    tr.rng._iter(hard.device).fill_(7)
    c0 = _launches()
    d_loss = tr.critic.loss_and_grad(loc, vox, hard, soft, tr.rng)
    torch.cuda.synchronize()
    c1 = _launches()
    g_loss, g_hard = tr._gen_iteration(loc, vox)
    torch.cuda.synchronize()
    c2 = _launches()
    assert tr.critic.__dict__.get("native_calls", 0) == 1 and tr.gen_engine.__dict__.get("native_calls", 0) == 1
    out = {"d_loss": d_loss.detach().cpu().clone(), "gp": tr.critic.last_gp.detach().cpu().clone(),
           "d_grad": tr.flat_d.grad.cpu().clone(), "g_loss": g_loss.detach().cpu().clone(),
           "g_hard": g_hard.detach().cpu().clone(), "g_grad": tr.flat_g.grad.cpu().clone(),
           "critic_chains": c1 - c0, "gen_chains": c2 - c1}
    if path:
        torch.save(out, path)
    return out


def _engine_run(knob):
    """engine_outputs with VG_GEMM_CHAIN = knob: here if that is this process's setting, else in a child."""
    if os.environ.get("VG_GEMM_CHAIN", "1") == knob:
        return engine_outputs()
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.pt")
        code = ("import sys; sys.path.insert(0, %r); import conftest, test_mlp_chain_gpu as t; t.engine_outputs(%r)"
                % (here, path))
        proc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VG_GEMM_CHAIN=knob), capture_output=True,
                              text=True, timeout=300)
        assert proc.returncode == 0, proc.stdout + proc.stderr
        return torch.load(path)


def test_engines_equal_with_the_chain_on_and_off(cuda):
    on, off = _engine_run("1"), _engine_run("0")
    # passes A, B tail, C head, D tail; D's forward head and input-VJP tail
    assert on["critic_chains"] == 4 and on["gen_chains"] == 2
    assert off["critic_chains"] == 0 and off["gen_chains"] == 0
    for k in ("d_loss", "gp", "d_grad", "g_loss", "g_hard", "g_grad"):
        assert torch.equal(on[k], off[k]), k
    assert bool(torch.isfinite(on["d_grad"]).all()) and float(on["d_grad"].abs().max()) > 0
    assert bool(torch.isfinite(on["g_grad"]).all()) and float(on["g_grad"].abs().max()) > 0


def test_policy_answers(cuda):
    """vg_gemm_chain_use: chains of 2 or 3 links only; never more tiles than one workgroup round holds."""
    from vgan._lib import LIB

    assert LIB.vg_gemm_chain_use(13000, 1) == 0 and LIB.vg_gemm_chain_use(13000, 4) == 0
    assert LIB.vg_gemm_chain_use(0, 2) == 0
    mode = os.environ.get("VG_GEMM_CHAIN", "1")
    if mode == "1":
        assert LIB.vg_gemm_chain_use(6400, 2) == 1 and LIB.vg_gemm_chain_use(6400, 3) == 1  # one tile per CU at most
        assert LIB.vg_gemm_chain_use(64 * 100000, 3) == 0
    elif mode == "0":
        assert LIB.vg_gemm_chain_use(6400, 3) == 0
