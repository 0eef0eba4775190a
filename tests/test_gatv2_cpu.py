"""GATV2CONV without a GPU: the restated semantics against an independent dense
form, model construction parity with the swapped oracle, the host-only argument
checks of the C ABI and the kernels' resource use (hipcc cross-compiles gfx950)."""
from __future__ import annotations

import ctypes as ct
import os
import re
import subprocess

import pytest
import torch

import gatv2_ref as V2
from oracle import reference as R
from parity_util import tiny_config
from vgan.config import Configuration
from vgan.models import VoxelGNNDiscriminator, VoxelGNNGenerator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "building-gan-graph-conditioned-architectural-volume-generation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
VG_EINVAL = -1
V2_PARAM_ORDER = ["att", "bias", "lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias"]


def test_sparse_restatement_matches_dense_form():
    torch.manual_seed(1)
    n = 40
    ei = V2.small_graph(n)
    assert int((ei[0] == ei[1]).sum()) == 2 and int((ei[1] == n - 1).sum()) == 0
    for c in (1, 5, 16):
        x_l, x_r = torch.randn(n, c, dtype=torch.float64), torch.randn(n, c, dtype=torch.float64)
        att, bias = torch.randn(c, dtype=torch.float64), torch.randn(c, dtype=torch.float64)
        a = V2.gatv2_propagate(x_l, x_r, att, bias, ei)
        b = V2.gatv2_dense(x_l, x_r, att, bias, ei)
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
        # the node without incoming edges attends to itself alone
        assert torch.allclose(a[n - 1], x_l[n - 1] + bias, rtol=0, atol=1e-12)


def _cfg(tiny: bool, g_kind: str = "GATV2CONV", d_kind: str = "GATV2CONV"):
    cfg = Configuration()
    cfg.DEVICE = "cpu"
    if tiny:
        tiny_config(cfg)
    cfg.GENERATOR_CONV_TYPE, cfg.DISCRIMINATOR_CONV_TYPE = g_kind, d_kind
    return cfg


@pytest.mark.parametrize("tiny", [False, True])
def test_gatv2_models_construct_like_the_swapped_oracle(tiny):
    cfg = _cfg(tiny)
    torch.manual_seed(777)
    g_ref, d_ref = V2.build_v2(R.Generator, cfg), V2.build_v2(R.Discriminator, cfg)
    torch.manual_seed(777)
    g, d = VoxelGNNGenerator(cfg, 17, 12), VoxelGNNDiscriminator(cfg, 17, 12)
    for mine, ref in ((g, g_ref), (d, d_ref)):
        a, b = mine.state_dict(), ref.state_dict()
        assert list(a.keys()) == list(b.keys())
        assert [k for k, _ in mine.named_parameters()] == [k for k, _ in ref.named_parameters()]
        for k in a:
            assert a[k].shape == b[k].shape, k
            assert torch.equal(a[k], b[k]), k
        conv0 = [k[len("encoder.module_0."):] for k, _ in mine.named_parameters() if k.startswith("encoder.module_0.")]
        assert conv0 == V2_PARAM_ORDER
        c = mine.encoder.module_0.out_channels
        assert tuple(a["encoder.module_0.att"].shape) == (1, 1, c)
        assert tuple(a["encoder.module_0.lin_r.weight"].shape) == (c, mine.encoder.module_0.in_channels)
    # the swapped oracle (fresh draws) carries the same keys and shapes, and
    # state dicts load both ways
    sw = V2.swap_convs(R.Generator(cfg))
    assert {k: v.shape for k, v in sw.state_dict().items()} == {k: v.shape for k, v in g.state_dict().items()}
    sw.load_state_dict(g.state_dict())
    g2 = VoxelGNNGenerator(cfg, 17, 12)
    g2.load_state_dict(sw.state_dict())
    for k, v in g.state_dict().items():
        assert torch.equal(v, g2.state_dict()[k]), k
    d2 = VoxelGNNDiscriminator(cfg, 17, 12)
    d2.load_state_dict(V2.swap_convs(R.Discriminator(cfg)).state_dict())


def test_mixed_conv_types_construct():
    g = VoxelGNNGenerator(_cfg(True, "GATV2CONV", "GATCONV"), 17, 12)
    d = VoxelGNNDiscriminator(_cfg(True, "GATV2CONV", "GATCONV"), 17, 12)
    assert "encoder.module_0.att" in g.state_dict() and "encoder.module_0.att_src" in d.state_dict()


@pytest.mark.parametrize("kind,exc", [("GCNCONV", NotImplementedError), ("GRAPHCONV", NotImplementedError),
                                      ("FOO", ValueError)])
def test_other_conv_types_are_refused(kind, exc):
    with pytest.raises(exc):
        VoxelGNNGenerator(_cfg(True, g_kind=kind), 17, 12)
    with pytest.raises(exc):
        VoxelGNNDiscriminator(_cfg(True, d_kind=kind), 17, 12)


def test_gatv2_abi_checks_arguments_on_the_host():
    """Every refusal happens before any launch: the pointers below are not
    device addresses (and no GPU is present here)."""
    from vgan._lib import LIB as lib

    p = 256  # a non-NULL stand-in; never dereferenced on these paths

    def fwd(n=10, c=16, ld_l=16, ld_r=16, xl=p, alpha=p):
        return lib.vg_gatv2_fwd(p, p, n, c, xl, ld_l, p, ld_r, p, p, 0.2, p, alpha, None)

    def bwd(n=10, e=30, c=16, ld_l=16, ld_r=16, ld_gl=16, ld_gr=16, g_att=p, g_bias=p, ws=p, g_out=p):
        return lib.vg_gatv2_bwd(p, p, p, p, p, n, e, c, p, ld_l, p, ld_r, p, p, g_out, 0.2, p, ld_gl, p, ld_gr, g_att,
                                g_bias, 0, ws, None)

    for f in (fwd, bwd):
        assert f(n=0) == VG_EINVAL
        assert f(c=257) == VG_EINVAL and f(c=0) == VG_EINVAL
        assert f(ld_l=15) == VG_EINVAL and f(ld_r=15) == VG_EINVAL
    assert fwd(xl=None) == VG_EINVAL and fwd(alpha=None) == VG_EINVAL
    assert bwd(ws=None) == VG_EINVAL and bwd(g_out=None) == VG_EINVAL
    assert bwd(ld_gl=15) == VG_EINVAL and bwd(ld_gr=15) == VG_EINVAL
    assert bwd(e=0) == VG_EINVAL
    assert bwd(g_att=None) == VG_EINVAL  # g_att / g_bias: both or neither


def test_gatv2_workspace_query():
    from vgan._lib import LIB as lib

    sizes = [int(lib.vg_gatv2_bwd_ws_floats(1000, e, 64)) for e in (1, 1000, 9000, 27000)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert sizes[2] >= 9000  # ge [E'] lives there


def _usage(src: str) -> dict:
    """{kernel mangled name: {"vgpr", "occ", "lds", "spill"}} of one source."""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-pass-failed",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", os.devnull],
                         capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("spill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return res


def test_gatv2_kernels_spill_nothing_and_hold_one_partials_image():
    table = _usage("gatv2.hip")
    kernels = {k: v for k, v in table.items() if "k_gatv2_" in k}
    # forward, destination pass and source pass in 11 row shapes each, and the fold
    assert len(kernels) >= 3 * 11 + 1, sorted(kernels)
    for name, u in sorted(kernels.items()):
        print(f"{name}: {u}")  # occupancy is recorded in DESIGN.md, not asserted (no measured target)
        assert u.get("spill", 0) == 0, (name, u)
        assert u["lds"] <= 16384, (name, u)
