"""tests/tools/device_io.py itself: the byte arithmetic of the read-back and of the sentinel tensors.
The sizes are odd on purpose."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import device_io as D  # noqa: E402
from support import assert_bits  # noqa: E402

pytestmark = pytest.mark.gpu


def test_download_gives_the_tensors_bytes():
    import torch
    five = torch.tensor([1.5, -0.0, float("nan"), 3e-41, -7.0], dtype=torch.float32, device="cuda:0")
    texels = (torch.arange(21, dtype=torch.int32, device="cuda:0") * 11).to(torch.uint8).reshape(3, 7)
    torch.cuda.synchronize()
    assert_bits(D.download(five.data_ptr(), (5,)), five.cpu().numpy(), "5 floats")
    assert_bits(D.download(texels.data_ptr(), (3, 7), np.uint8), texels.cpu().numpy(), "3 x 7 bytes")
    assert D.download(0, (5,)) is None and D.download(None, (3, 7), np.uint8) is None


def test_the_runtime_handle_is_made_once():
    assert D.hip_runtime() is D.hip_runtime()


def test_filled_tensors_hold_the_value():
    import torch
    t = D.filled((2, 3, 3), -7.0, torch.float32)
    assert t.device.type == "cuda" and t.dtype == torch.float32 and tuple(t.shape) == (2, 3, 3)
    assert (t.cpu().numpy() == np.float32(-7.0)).all()
    assert tuple(D.plane(5, 3, 1).shape) == (3, 5) and tuple(D.plane(5, 3, 2, torch.int32).shape) == (3, 5, 2)
    out = D.Outputs(5, 3, own_stream=False)
    rgb, rgb8 = out.host()
    assert (rgb == D.SENTINEL).all() and rgb.shape == (3, 5, 3) and (rgb8 == D.TEXEL).all() and rgb8.dtype == np.uint8
    assert D.Outputs(5, 3, f32=False, own_stream=False).host()[0] is None
