"""The BCE objective (USE_WGANGP = False) without a GPU: the host-only argument
checks of the new C entry points, the head's workspace query, model
construction parity with the oracle, and the new kernels' resource use (hipcc
cross-compiles gfx950)."""
from __future__ import annotations

import os
import re
import subprocess

import pytest
import torch.nn as nn

from oracle import reference as R
from parity_util import tiny_config
from vgan.config import Configuration
from vgan.models import VoxelGNNDiscriminator, VoxelGNNGenerator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "building-gan-graph-conditioned-architectural-volume-generation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
VG_EINVAL = -1


def test_bce_abi_checks_arguments_on_the_host():
    """Every refusal happens before any launch: the pointers below are not
    device addresses (and no GPU is present here)."""
    from vgan._lib import LIB as lib

    p = 256  # a non-NULL stand-in; never dereferenced on these paths

    def head(n=10, s=p, out=p, seeds=p, ws=p, sync=p):
        return lib.vg_bce_critic_head(s, n, out, seeds, ws, sync, None)

    assert head(n=0) == VG_EINVAL and head(n=-3) == VG_EINVAL
    for name in ("s", "out", "seeds", "ws", "sync"):
        assert head(**{name: None}) == VG_EINVAL, name

    def fwd(n=10, k=7, g=2, d_fake=p, out=p, ws=p):
        return lib.vg_gen_loss_bce_fwd(d_fake, p, p, p, p, n, k, p, p, g, 1.0, 1.0, 1.0, 1.0, 1.0, out, ws, None)

    def bwd(n=10, k=7, g_loss=p, out=p, d_fake=p, logits=p, g_dfake=p, g_logits=p):
        return lib.vg_gen_loss_bce_bwd(g_loss, out, d_fake, logits, p, n, k, g_dfake, p, g_logits, None)

    assert fwd(n=0) == VG_EINVAL and fwd(k=2) == VG_EINVAL and fwd(k=33) == VG_EINVAL and fwd(g=0) == VG_EINVAL
    assert fwd(d_fake=None) == VG_EINVAL and fwd(out=None) == VG_EINVAL and fwd(ws=None) == VG_EINVAL
    assert bwd(n=0) == VG_EINVAL and bwd(k=0) == VG_EINVAL and bwd(k=33) == VG_EINVAL
    assert bwd(g_loss=None) == VG_EINVAL and bwd(out=None) == VG_EINVAL
    assert bwd(d_fake=None) == VG_EINVAL  # the adversarial gradient needs each row's score
    assert bwd(logits=None) == VG_EINVAL  # g_logits wanted
    # the stacked input of two copies needs neither soft labels nor eps; three copies do
    assert lib.vg_critic_input(p, 10, 5, p, p, None, None, 7, 3, p, None) == VG_EINVAL
    assert lib.vg_critic_input(p, 10, 5, p, p, None, None, 7, 1, p, None) == VG_EINVAL
    assert lib.vg_critic_input(p, 0, 5, p, p, None, None, 7, 2, p, None) == VG_EINVAL
    assert lib.vg_critic_input(p, 10, 5, p, None, None, None, 7, 2, p, None) == VG_EINVAL


def test_bce_head_workspace_query_is_monotone():
    from vgan._lib import LIB as lib

    sizes = [int(lib.vg_bce_critic_head_ws_floats(n)) for n in (1, 64, 256, 257, 1000, 20001, 300000)]
    assert sizes[0] >= 2 and sizes == sorted(sizes)
    assert sizes[3] > sizes[2] and sizes[-1] > sizes[-2]


def test_bce_models_have_the_oracle_keys_and_end_in_sigmoid():
    cfg = tiny_config(Configuration())
    cfg.DEVICE = "cpu"
    cfg.USE_WGANGP = False
    D = VoxelGNNDiscriminator(cfg, 17, 12)
    Do = R.Discriminator(cfg)
    ours = {k: tuple(v.shape) for k, v in D.state_dict().items()}
    theirs = {k: tuple(v.shape) for k, v in Do.state_dict().items()}
    assert ours == theirs
    assert isinstance(list(D.decoder.children())[-1], nn.Sigmoid)
    assert isinstance(list(Do.decoder.children())[-1], nn.Sigmoid)
    Do.load_state_dict(D.state_dict())
    # both engines accept this configuration; the WGAN-GP engine still refuses it
    from vgan.bce import BceCriticEngine, bce_decoder_ok
    from vgan.critic import CriticEngine
    from vgan.genstep import GeneratorEngine

    assert bce_decoder_ok(D)
    BceCriticEngine(D, cfg)
    with pytest.raises(ValueError, match="USE_WGANGP=True"):
        CriticEngine(D, cfg)
    G = VoxelGNNGenerator(cfg, 17, 12)
    assert GeneratorEngine(G, D, cfg).supported
    cfg.USE_WGANGP = True
    D_w = VoxelGNNDiscriminator(cfg, 17, 12)
    assert not bce_decoder_ok(D_w)
    with pytest.raises(ValueError, match="USE_WGANGP=False"):
        BceCriticEngine(D_w, cfg)
    cfg.USE_WGANGP = False
    assert not GeneratorEngine(G, D_w, cfg).supported  # BCE needs the trailing Sigmoid


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


def test_bce_kernels_spill_nothing():
    """The critic head (bce.hip) and every instantiation of the generator loss
    head (head.hip: the BCE ones are new, the WGAN-GP ones now share their
    device code through a template flag)."""
    head = {k: v for k, v in _usage("bce.hip").items() if "k_bce_critic_head" in k}
    assert len(head) == 1, sorted(head)
    gen = {k: v for k, v in _usage("head.hip").items() if "k_gen_loss_" in k}
    # partial <8 | 32> x <WGAN | BCE>, final and backward x <WGAN | BCE>
    assert len(gen) == 8, sorted(gen)
    assert sum("Lb1E" in k for k in gen) == 4, sorted(gen)
    for name, u in sorted({**head, **gen}.items()):
        print(f"{name}: {u}")  # occupancy is printed, not asserted (latency kernels, no measured target)
        assert u.get("spill", 0) == 0, (name, u)
