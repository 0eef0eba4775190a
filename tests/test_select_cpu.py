"""Best-of-k selection, the parts that need no GPU: metrics.macro_f1 against
metrics.scores, vg_sweep_select's host-side argument checks (VG_EINVAL before
any runtime call, no device pointer involved) and the wrapper's refusal of CPU
tensors."""
import numpy as np
import pytest

VG_EINVAL = -1


def test_macro_f1_equals_scores_per_matrix():
    from vgan import metrics

    rng = np.random.default_rng(7)
    conf = rng.integers(0, 50, size=(3, 4, 7, 7))
    conf[0, 0] = 0  # an empty building
    conf[1, 2, 3, :] = 0  # a label absent from the truth ...
    conf[1, 2, :, 3] = 0  # ... and from the prediction: outside the label set
    conf[2, 1] = np.diag(np.arange(7))  # perfect, label 0 absent
    got = metrics.macro_f1(conf)
    assert got.shape == (3, 4) and got.dtype == np.float64
    want = np.array([[metrics.scores(conf[i, j])[0] for j in range(4)] for i in range(3)])
    # the same divisions; only the order of a sum of <= 7 terms in [0, 1] may differ
    assert np.abs(got - want).max() <= 1e-15
    assert got[0, 0] == 0.0 and got[2, 1] == 1.0
    assert metrics.macro_f1(np.zeros((7, 7), dtype=np.int32)) == 0.0
    assert metrics.macro_f1(np.zeros((2, 5, 5))).tolist() == [0.0, 0.0]


def _call(lib, **kw):
    """vg_sweep_select with made-up non-NULL addresses (never dereferenced: the
    checks under test return before any launch) and one argument replaced."""
    a = dict(pred=8, copy_stride=100, copies=3, truth=8, classes=7, ptr=8, num_graphs=2, x=8, x_stride=12,
             site_area=8, far_col=9, dy_col=4, dx_col=5, dim_scale=11.0, void_class=6, criterion=0, conf=8, f1=8,
             far_gen=8, far_ref=8, best=8, labels=8, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.vg_sweep_select(*a.values())


def test_sweep_select_refuses_bad_arguments_host_only():
    from vgan import _lib
    from vgan._lib import LIB as lib

    assert _lib.VG_SELECT_MAX_COPIES == 64 and (_lib.VG_SELECT_F1, _lib.VG_SELECT_FAR) == (0, 1)
    for name in ("pred", "ptr", "x", "site_area", "best"):
        assert _call(lib, **{name: None}) == VG_EINVAL, name
    for copies in (0, -1, _lib.VG_SELECT_MAX_COPIES + 1):
        assert _call(lib, copies=copies) == VG_EINVAL, copies
    for classes in (0, -3, 33):
        assert _call(lib, classes=classes) == VG_EINVAL, classes
    # copies * classes^2 * 4 bytes of LDS counters: 17 * 32^2 * 4 > 64 KB >= 16 * 32^2 * 4
    assert _call(lib, copies=17, classes=32) == VG_EINVAL
    assert _call(lib, copies=64, classes=17) == VG_EINVAL
    for criterion in (-1, 2):
        assert _call(lib, criterion=criterion) == VG_EINVAL, criterion
    # no ground truth: the F1 criterion, conf and f1 cannot be served
    assert _call(lib, truth=None, criterion=_lib.VG_SELECT_F1, conf=None, f1=None) == VG_EINVAL
    assert _call(lib, truth=None, criterion=_lib.VG_SELECT_FAR, f1=None) == VG_EINVAL
    assert _call(lib, truth=None, criterion=_lib.VG_SELECT_FAR, conf=None) == VG_EINVAL
    assert _call(lib, num_graphs=0) == VG_EINVAL


def test_header_states_the_candidate_limit():
    import os
    import re

    from parity_util import ROOT
    from vgan import _lib

    hdr = open(os.path.join(ROOT, "include", "vgan.h")).read()
    assert int(re.search(r"#define VG_SELECT_MAX_COPIES (\d+)", hdr).group(1)) == _lib.VG_SELECT_MAX_COPIES == 64
    assert int(re.search(r"#define VG_SELECT_F1 (\d+)", hdr).group(1)) == _lib.VG_SELECT_F1
    assert int(re.search(r"#define VG_SELECT_FAR (\d+)", hdr).group(1)) == _lib.VG_SELECT_FAR


def test_sweep_select_refuses_cpu_tensors():
    import torch

    from vgan import ops

    n = 5
    pred = torch.zeros(2, n, dtype=torch.int8)
    ptr = torch.tensor([0, n])
    x = torch.zeros(n, 12)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.sweep_select(pred, ptr, x, torch.ones(n), truth=torch.zeros(n, dtype=torch.long))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.sweep_select(pred, ptr, x, torch.ones(n), criterion="far")
    with pytest.raises(ValueError, match="criterion"):
        ops.sweep_select(pred, ptr, x, torch.ones(n), criterion="iou")


def test_sweep_keyword_is_validated_before_any_batch():
    """run / run_stream refuse an unknown ``select`` before touching a batch
    (no model or device needed to reach the check)."""
    from vgan.infer import InferenceSweep

    sw = InferenceSweep.__new__(InferenceSweep)
    for fn in (sw.run, sw.run_stream):
        with pytest.raises(ValueError, match="select"):
            fn(iter(()), select="iou")
