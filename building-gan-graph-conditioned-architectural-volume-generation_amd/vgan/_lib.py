"""ctypes binding of ``libvgan_hip.so`` (the C ABI declared in ``include/vgan.h``).

The binding is READ FROM THE HEADER at import (``vgan/_abi.py``): every
``VG_*`` integer ``#define``, one ``ctypes.Structure`` per ``typedef struct``
(``vg_gen_ln_layer`` -> ``VgGenLnLayer``; fields in header order under their
header names, ``in`` spelled ``in_``; pointer fields ``c_void_p``) and the
restype / argtypes of every prototype (a pointer to a header struct is
``POINTER(<mirror>)``, every other pointer ``c_void_p``).  A new entry point is
declared in ``include/vgan.h`` and defined in ``csrc/``; there is no third
place.  The header is therefore required next to the package, as it is to
build the library.

The library is REQUIRED: importing this module raises if it was not built, and
every wrapper refuses non-CUDA tensors.  There is no CPU or eager-torch fallback
for the message-passing core.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import _abi

# VGAN_LIB: an alternative build of the same ABI (A/B timing of kernel variants)
LIB_PATH = os.environ.get("VGAN_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvgan_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                           "include", "vgan.h")

_ABI = _abi.read(HEADER_PATH)
# VG_EINVAL, VG_SELECT_*, VG_FOLD_MAX, VG_*_GROUP_MAX, VG_*_MAX_LAYERS / _BLOCKS, ...
globals().update(_ABI.constants)
# VgFoldSrc, VgFold, VgTn, VgJvpSrc, VgGnBwdIn, VgDxIn, VgDrawTail, VgGnApply, VgGnJvp, VgChainLayer, VgGemmLink,
# VgCriticLinear ... VgCriticBatch, VgCsrRef, VgGenLnLayer ... VgGenStack, VgHgen*, VgHcritic*
globals().update({_cls.__name__: _cls for _cls in _ABI.structs.values()})
VgASrc = VgAsrc  # vg_asrc: the one name that is not the CamelCase of its C name
# name -> (restype, argtypes) of every function include/vgan.h declares
SIGNATURES = _ABI.signatures

# the dense products of the path, each also exported with bf16 operands
# (include/vgan.h, "bf16 training"); same signatures
DENSE = ("vg_gemm", "vg_gemm_tn", "vg_gemm_tn_deferred", "vg_gemm_tn_plan", "vg_gemm_ln_act", "vg_gemm_ln_act_ms",
         "vg_gat_lin_att", "vg_gemm_gn_bwd")

# VGAN_FOLD_BATCH: folds per vg_fold_batch launch (<= VG_FOLD_MAX; 40 was the round-4 limit, A/B knob)
_FOLD_BATCH = max(1, min(int(os.environ.get("VGAN_FOLD_BATCH", str(VG_FOLD_MAX))), VG_FOLD_MAX))
# VGAN_TN_GROUP=0: launch every weight-gradient product where the backward
# forms it (one launch per layer) instead of grouping them (A/B knob)
_TN_GROUP = os.environ.get("VGAN_TN_GROUP", "1") == "1"
# VGAN_JVP_GROUP=1: the tangent sweep's source passes as one grouped launch
# before pass D.  Off: measured 0.07 ms per step slower than one launch per
# block right after its destination-row pass
_JVP_GROUP = os.environ.get("VGAN_JVP_GROUP", "0") == "1"
# folds of more than 768 partial rows in two levels (vg_fold_batch_split),
# as the critic engine does; 0: vg_fold_batch
_FOLD_SPLIT = os.environ.get("VGAN_FOLD_SPLIT", "1") == "1"
# VGAN_GN_ROWS=0: the GraphNorm backward's elementwise pass as its own launch
# instead of in the GAT backward's destination-row pass (A/B knob)
_GN_ROWS = os.environ.get("VGAN_GN_ROWS", "1") == "1"
# VGAN_GN_APPLY_GEMM=1: the GraphNorm that ends a critic-engine block applied
# in the next block's projection GEMM (vg_gat_lin_att_gn) instead of by its own
# launch.  Off: measured slower (profiles/r02_ab_gn_apply_gemm.txt).
_GN_APPLY_GEMM = os.environ.get("VGAN_GN_APPLY_GEMM", "0") == "1"
# VGAN_GN_JVP_FUSE=1: the tangent sweep's GraphNorm sums formed in the GAT
# tangent pass (vg_gat_jvp2_gn_deferred) instead of their own pass.  Off:
# measured slower (k_jvp_rows 94 -> 154 VGPRs; profiles/r02_rejected_gn_jvp_fuse.txt)
_GN_JVP_FUSE = os.environ.get("VGAN_GN_JVP_FUSE", "0") == "1"
# VGAN_CHAIN=0: the critic's decoder chains as one vg_gemm launch per layer
# instead of one vg_linear_chain launch per pass (A/B knob)
_CHAIN = os.environ.get("VGAN_CHAIN", "1") == "1"


def linear_chain(x, ldx: int, rows: int, widths, layers, stream) -> bool:
    """vg_linear_chain over ``layers`` (dicts of VgChainLayer fields; device
    pointers as ints / c_void_p); False when the width chain has no kernel
    (the caller runs its per-layer GEMMs).  Only VG_EINVAL (no kernel for
    this width chain / alignment) falls back; a launch error raises."""
    if not _CHAIN:
        return False
    n = len(layers)
    arr = (VgChainLayer * n)()
    for i, l in enumerate(layers):
        for k, v in l.items():
            setattr(arr[i], k, v.value if isinstance(v, ctypes.c_void_p) else v)
    w = (ctypes.c_int32 * (n + 1))(*widths)
    name = "vg_linear_chain_bf16" if _precision == "bf16" else "vg_linear_chain"
    rc = getattr(LIB, name)(x, ldx, rows, w, n, arr, stream)
    if rc == VG_EINVAL:
        return False
    check(rc, name)
    return True


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The HIP library is required; there is no fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _check_stamp(lib)
    return lib


def source_hash(csrc: str) -> Optional[str]:
    """The hash csrc/Makefile stamps into the library: sha256 over csrc/*.hip,
    csrc/*.h and include/vgan.h concatenated in sorted path order (make's
    $(sort) of the relative paths), first 16 hex digits.  None when the
    sources are not in the tree."""
    import glob
    import hashlib

    if not os.path.isdir(csrc):
        return None
    rel = [os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))]
    rel.append("../../include/vgan.h")
    h = hashlib.sha256()
    for r in sorted(rel):
        path = os.path.normpath(os.path.join(csrc, r))
        if not os.path.exists(path):
            return None
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _check_stamp(lib) -> None:
    """A library built from other sources than the tree's fails loudly (a
    stale prebuilt .so would otherwise run old kernels under new tests).
    An explicit VGAN_LIB (an A/B build of other sources, tools/ab_libs.sh)
    is exempt."""
    if os.environ.get("VGAN_LIB"):
        return
    stamp = lib.vg_build_stamp().decode()
    want = source_hash(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc"))
    if want is not None and stamp.split(" ")[0] != want:
        raise ImportError(f"{LIB_PATH} was built from other sources (stamp {stamp.split(' ')[0]}, tree {want}): "
                          "rebuild it (make -C building-gan-graph-conditioned-architectural-volume-generation_amd/csrc)")


def build_stamp() -> str:
    """'<source hash> <hipcc version>' of the loaded library."""
    return LIB.vg_build_stamp().decode()


LIB = _load()


# Operand precision of the dense products: "f32" (the reference's) or "bf16"
# (configs[2]: bf16 operands, f32 accumulation and outputs).  A process-wide
# setting rather than a thread-local one: autograd runs the backward of the
# HIP ops on its own device thread, which must see the same precision.
PRECISIONS = ("f32", "bf16")
_precision = "f32"


def gemm_precision() -> str:
    return _precision


def set_gemm_precision(p: str) -> None:
    global _precision
    if p not in PRECISIONS:
        raise ValueError(f"gemm precision must be one of {PRECISIONS}, not {p!r}")
    _precision = p


class gemm_precision_scope:
    """``with gemm_precision_scope("bf16"): ...`` -- set, then restore."""

    def __init__(self, p: str):
        self.p = p

    def __enter__(self):
        self.prev = _precision
        set_gemm_precision(self.p)
        return self

    def __exit__(self, *exc):
        set_gemm_precision(self.prev)
        return False


def dense(name: str):
    """Entry point of the dense product ``name`` (one of DENSE) in the current precision."""
    return getattr(LIB, name + "_bf16" if _precision == "bf16" else name)


def ptr(t: Optional[torch.Tensor]):
    """A tensor's device address for a c_void_p argument: a plain int (ctypes
    converts it itself; wrapping every pointer in a c_void_p object cost ~0.4
    us each, ~4 us per ABI call of the eager paths' ~10 pointers), None for NULL."""
    return None if t is None else t.data_ptr()


def stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


_SYNC = {}


# measured slower at batch 32 (16.1 vs 18.2 ms/step: one contended counter for
# ~640 blocks), so off unless VGAN_LAST_BLOCK_FOLD=1
_LAST_BLOCK = os.environ.get("VGAN_LAST_BLOCK_FOLD", "0") == "1"


def sync_counter(device: torch.device):
    """Persistent zeroed int32 device counter per (device, current stream) for
    the kernels' last-block fold (left at 0 by every launch); None (separate
    finalize launches) when VGAN_LAST_BLOCK_FOLD=0."""
    if not _LAST_BLOCK:
        return None
    key = (torch.device(device), torch.cuda.current_stream(device).cuda_stream)
    t = _SYNC.get(key)
    if t is None:
        t = _SYNC[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return ptr(t)


def check(rc: int, name: str) -> None:
    if rc != 0:
        what = "invalid argument" if rc == VG_EINVAL else f"hipError {rc}"
        raise RuntimeError(f"{name} failed: {what}")


def require_cuda(*tensors: Optional[torch.Tensor]) -> None:
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("vgan HIP ops require tensors on a ROCm device (no CPU fallback)")
        if not t.is_contiguous():
            raise RuntimeError("vgan HIP ops require contiguous tensors")


class FoldCollector:
    """Collects the parameter-gradient folds of one backward (the *_deferred
    ABI calls) and runs them in as few vg_fold_batch launches as possible.
    Folds into the same destination merge into one two-source fold, applied
    in call order ((out + first) + second, as the immediate folds would); the
    partial workspaces are kept alive until the batch is enqueued."""

    def __init__(self):
        self.folds = []
        self.keep = []
        self.products = []
        self.jvp_src = []

    def call(self, fn, args_before_stream, stream, keep=(), name="deferred"):
        arr = (VgFold * 3)()
        n = ctypes.c_int32(0)
        check(fn(*args_before_stream, arr, ctypes.byref(n), stream), name)
        for i in range(n.value):
            self.folds.append(VgFold.from_buffer_copy(arr[i]))
        self.keep.extend(keep)

    def tn(self, args_before_outputs, stream, keep=()):
        """A weight-gradient product (vg_gemm_tn_plan's arguments up to the
        workspace; accumulate into C / db).  It runs at flush() in one
        vg_gemm_tn_group launch with the backward's other products, before
        the folds; ``keep`` holds A, B and the workspace until then."""
        if not _TN_GROUP:
            self.call(dense("vg_gemm_tn_deferred"), args_before_outputs, stream, keep=keep, name="vg_gemm_tn_deferred")
            return
        prod = VgTn()
        arr = (VgFold * 2)()
        n = ctypes.c_int32(0)
        check(dense("vg_gemm_tn_plan")(*args_before_outputs, ctypes.byref(prod), arr, ctypes.byref(n)),
              "vg_gemm_tn_plan")
        self.products.append(prod)
        for i in range(n.value):
            self.folds.append(VgFold.from_buffer_copy(arr[i]))
        self.keep.extend(keep)

    def jvp(self, args_before_outputs, stream, keep=()):
        """vg_gat_jvp2 with its folds deferred and its source pass (dQ/dh
        injections) described for ONE grouped launch by run_jvp_src();
        ``keep`` holds h, u, g_out and the workspace until then."""
        arr = (VgFold * 2)()
        n = ctypes.c_int32(0)
        if not _JVP_GROUP:
            check(LIB.vg_gat_jvp2_deferred(*args_before_outputs, arr, ctypes.byref(n), stream), "vg_gat_jvp2_deferred")
        else:
            src = VgJvpSrc()
            check(LIB.vg_gat_jvp2_plan(*args_before_outputs, arr, ctypes.byref(n), ctypes.byref(src), stream),
                  "vg_gat_jvp2_plan")
            if src.shape >= 0:
                self.jvp_src.append(src)
        for i in range(n.value):
            self.folds.append(VgFold.from_buffer_copy(arr[i]))
        self.keep.extend(keep)

    def jvp_gn(self, args_before_outputs, gn: "VgGnJvp", stream, keep=()):
        """vg_gat_jvp2_gn_deferred: ``jvp`` (source pass run here) that also
        writes the GraphNorm tangent sums of ``gn`` into gn.part."""
        arr = (VgFold * 2)()
        n = ctypes.c_int32(0)
        check(LIB.vg_gat_jvp2_gn_deferred(*args_before_outputs, ctypes.byref(gn), arr, ctypes.byref(n), stream),
              "vg_gat_jvp2_gn_deferred")
        for i in range(n.value):
            self.folds.append(VgFold.from_buffer_copy(arr[i]))
        self.keep.extend(keep)

    def run_jvp_src(self, stream) -> None:
        """The described source passes, in one launch per VG_JVP_GROUP_MAX."""
        for i in range(0, len(self.jvp_src), VG_JVP_GROUP_MAX):
            part = self.jvp_src[i:i + VG_JVP_GROUP_MAX]
            arr = (VgJvpSrc * len(part))(*part)
            check(LIB.vg_gat_jvp_src_group(arr, len(part), stream), "vg_gat_jvp_src_group")
        self.jvp_src = []

    def _launch_products(self, stream) -> None:
        for bf in (0, 1):
            prods = [p for p in self.products if p.bf16 == bf]
            for i in range(0, len(prods), VG_TN_GROUP_MAX):
                part = prods[i:i + VG_TN_GROUP_MAX]
                arr = (VgTn * len(part))(*part)
                check(LIB.vg_gemm_tn_group(arr, len(part), stream), "vg_gemm_tn_group")
        self.products = []

    def flush(self, stream) -> None:
        self.run_jvp_src(stream)  # (their att_src partials feed folds)
        # the grouped products first: their partials feed the folds
        self._launch_products(stream)
        batches, cur, where = [], [], {}
        for f in self.folds:
            j = where.get(f.out)
            if j is not None:
                g = cur[j]
                if (g.nsrc == 1 and f.nsrc == 1 and f.accumulate and (g.width, g.k, g.ldo) == (f.width, f.k, f.ldo)):
                    g.src[1] = f.src[0]
                    g.nsrc = 2
                    continue
                batches.append(cur)  # cannot merge: later batch, so the two never race
                cur, where = [], {}
            if len(cur) == _FOLD_BATCH:
                batches.append(cur)
                cur, where = [], {}
            where[f.out] = len(cur)
            cur.append(f)
        if cur:
            batches.append(cur)
        for b in batches:
            arr = (VgFold * len(b))(*b)
            need = int(LIB.vg_fold_split_ws_floats(arr, len(b))) if _FOLD_SPLIT else 0
            if need > 0:  # the chunk sums' workspace, on the current stream (the folds' own: stream-ordered reuse)
                ws = torch.empty(need, dtype=torch.float32, device="cuda")
                check(LIB.vg_fold_batch_split(arr, len(b), ws.data_ptr(), need, stream), "vg_fold_batch_split")
            else:
                check(LIB.vg_fold_batch(arr, len(b), stream), "vg_fold_batch")
        self.folds, self.keep = [], []
