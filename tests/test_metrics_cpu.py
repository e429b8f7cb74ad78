"""CPU tests of the completion-metrics host layer (shapeformer_amd/metrics.py): argument checks that must fire before any launch,
and the callback flag's default.  No GPU."""
import inspect

import numpy as np
import pytest
import torch


def test_cpu_tensors_raise_before_any_launch():
    from shapeformer_amd import metrics as M
    from shapeformer_amd._lib import SfmiError
    p, q = torch.rand(10, 3), torch.rand(12, 3)
    with pytest.raises(SfmiError):
        M.nn_dist(p, q)
    with pytest.raises(SfmiError):
        M.nn_dist(p[None], q[None], return_index=True)
    with pytest.raises(SfmiError):
        M.tmd([p, q])
    with pytest.raises(SfmiError):
        M.uhd(p, torch.rand(2, 7, 3))
    v, f = torch.rand(4, 3), torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    with pytest.raises(SfmiError):
        M.sample_mesh_dev(v, f, [0, 4], [0, 2], 16, seed=1)
    with pytest.raises(SfmiError):
        M.nn_dist(p.numpy(), q)                      # not a tensor


@pytest.mark.parametrize("p_off,q_off", [
    ([1, 10], [0, 12]),              # does not start at 0
    ([0, 9], [0, 12]),               # does not end at N
    ([0, 6, 4, 10], [0, 4, 8, 12]),  # decreasing
    ([0, 5, 10], [0, 12]),           # different set counts
    ([0, 5, 10], [0, 12, 12]),       # an empty reference set with queries
    ([[0, 10]], [[0, 12]]),          # not 1-D
    ([0.0, 10.0], [0, 12]),          # not integer
])
def test_malformed_offsets_raise(p_off, q_off):
    from shapeformer_amd import metrics as M
    from shapeformer_amd._lib import SfmiError
    with pytest.raises(SfmiError):
        M.nn_dist(torch.rand(10, 3), torch.rand(12, 3), p_off=p_off, q_off=q_off)


def test_malformed_mesh_offsets_raise():
    from shapeformer_amd import metrics as M
    from shapeformer_amd._lib import SfmiError
    v, f = torch.rand(6, 3), torch.tensor([[0, 1, 2], [0, 1, 2]], dtype=torch.int32)
    for voff, toff in (([0, 3, 6], [0, 2, 2]),     # second shape without faces
                       ([0, 3, 6], [0, 2]),        # batch sizes disagree
                       ([0, 7], [0, 2])):          # does not end at V
        with pytest.raises(SfmiError):
            M.sample_mesh_dev(v, f, voff, toff, 8)
    with pytest.raises(SfmiError):
        M.sample_mesh_dev(v, f, [0, 6], [0, 2], -1)


def test_eval_metrics_is_off_by_default():
    from shapeformer_amd import callbacks as CB
    sig = inspect.signature(CB.VisShapeFormer.__init__)
    assert sig.parameters["eval_metrics"].default is False
    assert sig.parameters["eval_tau"].default == 0.01 and sig.parameters["eval_points"].default == 10 ** 5
    cb = CB.VisShapeFormer(end_tokens=(4096, 4096))
    assert cb.eval_metrics is False


def test_library_declares_the_metric_entry_points():
    from shapeformer_amd import _lib as L
    for name in ("sfmi_nn_dist_f32", "sfmi_nn_dist_workspace_bytes", "sfmi_mesh_sample_f32", "sfmi_mesh_sample_workspace_bytes"):
        assert name in L.PROTOTYPES
    lib = L.lib()
    # workspace sizes are pure host arithmetic: one 10^5 x 10^5 direction splits Q, a 90-direction batch does not
    assert lib.sfmi_nn_dist_workspace_bytes(1, 10 ** 5, 10 ** 5) > 10 ** 5 * 8
    assert lib.sfmi_nn_dist_workspace_bytes(90, 9 * 10 ** 6, 9 * 10 ** 6) < 4096
    assert lib.sfmi_mesh_sample_workspace_bytes(2, 1000) >= 8000
    assert np.isfinite(lib.sfmi_nn_dist_workspace_bytes(3, 0, 5))
