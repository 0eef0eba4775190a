"""GATv2Conv of torch_geometric 2.6.1 (``nn/conv/gatv2_conv.py``) restated in
plain torch on top of ``oracle.pyg`` (test-only CPU reference), with the
defaults the reference's models use: heads=1, concat=True, negative_slope=0.2,
dropout=0.0, add_self_loops=True, edge_dim=None, fill_value='mean', bias=True,
share_weights=False, residual=False.

    x_l = lin_l(x), x_r = lin_r(x)
    edges: remove self loops, append one loop per node (GATConv's edge set)
    e_k   = sum_c att_c leaky_relu(x_l[src_k] + x_r[dst_k])_c
    alpha = softmax of e over the edges of each destination (utils/_softmax.py)
    out_i = sum_{k: dst_k = i} alpha_k x_l[src_k] + bias

Three forms: ``gatv2_propagate`` (sparse, functional), ``GATv2Conv`` (the module:
state_dict keys, parameter order and construction draws of the package's) and
``gatv2_dense`` (an independent N x N masked softmax, for the CPU self-check).
``swap_convs`` / ``build_v2`` turn an ``oracle.reference`` model into its
GATV2CONV form.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import pyg


def gatv2_propagate(x_l: torch.Tensor, x_r: torch.Tensor, att: torch.Tensor, bias, edge_index: torch.Tensor,
                    slope: float = pyg.NEG_SLOPE) -> torch.Tensor:
    n, c = x_l.shape
    ei = pyg.add_self_loops(pyg.remove_self_loops(edge_index), n)
    src, dst = ei[0], ei[1]
    u = x_l.index_select(0, src) + x_r.index_select(0, dst)  # [E', C]
    e = (F.leaky_relu(u, slope) * att.reshape(1, c)).sum(-1)
    alpha = pyg.segment_softmax(e, dst, n)
    msg = alpha.unsqueeze(-1) * x_l.index_select(0, src)
    out = torch.zeros(n, c, dtype=msg.dtype, device=msg.device).index_add_(0, dst, msg)
    return out if bias is None else out + bias


def gatv2_dense(x_l: torch.Tensor, x_r: torch.Tensor, att: torch.Tensor, bias, edge_index: torch.Tensor,
                slope: float = pyg.NEG_SLOPE) -> torch.Tensor:
    """The same through an N x N adjacency mask (no duplicate edges): row i of
    the logit matrix is the destination, column j the source."""
    n, c = x_l.shape
    mask = torch.zeros(n, n, dtype=torch.bool)
    keep = edge_index[0] != edge_index[1]
    mask[edge_index[1][keep], edge_index[0][keep]] = True
    mask |= torch.eye(n, dtype=torch.bool)
    u = x_l.unsqueeze(0) + x_r.unsqueeze(1)  # [dst, src, C]
    e = (F.leaky_relu(u, slope) * att.reshape(1, 1, c)).sum(-1)
    e = e.masked_fill(~mask, float("-inf"))
    p = (e - e.max(dim=1, keepdim=True).values.detach()).exp() * mask
    alpha = p / (p.sum(dim=1, keepdim=True) + pyg.SOFTMAX_EPS)
    out = alpha @ x_l
    return out if bias is None else out + bias


class GATv2Conv(nn.Module):
    """Parameters ``att`` [1, 1, out], ``bias`` [out], ``lin_l.{weight,bias}``,
    ``lin_r.{weight,bias}`` (``parameters()`` yields them in this order: own
    parameters, then the children as registered).  Each Linear draws its
    weight in its constructor; ``reset_parameters`` draws both again, then
    ``att`` (glorot); the three biases are zeros."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, 1
        self.lin_l = pyg.Linear(in_channels, out_channels, bias=True)
        self.lin_r = pyg.Linear(in_channels, out_channels, bias=True)
        self.att = nn.Parameter(torch.empty(1, 1, out_channels))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        self.lin_l.reset_parameters()
        self.lin_r.reset_parameters()
        pyg.glorot(self.att)
        with torch.no_grad():
            self.bias.zero_()

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
        return gatv2_propagate(self.lin_l(x), self.lin_r(x), self.att, self.bias, edge_index)


def small_graph(n: int = 40, seed: int = 5) -> torch.Tensor:
    """n-node random graph without duplicate edges: two explicit self loops
    (nodes 3 and 17) and node n - 1 with no incoming edge but its loop."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (4 * n,), generator=g)
    dst = torch.randint(0, n - 1, (4 * n,), generator=g)  # nothing points at node n - 1
    keep = src != dst
    ei = torch.unique(torch.stack([src[keep], dst[keep]]), dim=1)
    return torch.cat([ei, torch.tensor([[3, 17], [3, 17]])], dim=1)


def swap_convs(model: nn.Module) -> nn.Module:
    """Every ``encoder.module_{4b}`` (a GATConv) of an ``oracle.reference``
    Generator / Discriminator replaced by a GATv2Conv of the same widths
    (``pyg.Sequential`` looks its modules up by name).  The new modules draw
    fresh initial values: load a state_dict afterwards."""
    enc = model.encoder
    for name, mod in list(enc.named_children()):
        if isinstance(mod, pyg.GATConv):
            setattr(enc, name, GATv2Conv(mod.in_channels, mod.out_channels))
    return model


@contextlib.contextmanager
def _v2_stack():
    keep = pyg.GATConv
    pyg.GATConv = GATv2Conv
    try:
        yield
    finally:
        pyg.GATConv = keep


def build_v2(factory, *args, **kwargs) -> nn.Module:
    """``factory(*args)`` (``oracle.reference.Generator`` / ``Discriminator``)
    constructed with GATv2Conv in place of GATConv, so the CPU generator is
    consumed in the order the reference's GATV2CONV models consume it."""
    with _v2_stack():
        return factory(*args, **kwargs)
