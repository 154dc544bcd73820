"""TEST INFRASTRUCTURE: the device-side helpers the GPU test modules share: reading a device address
back through the HIP runtime, sentinel-filled tensors, and the output images of a session call.

    from device_io import Outputs, download, filled, plane, read_planes

torch is imported where it is used, as in the test modules. Nothing here owns a scene or a session.
"""
import ctypes as C
import functools

import numpy as np

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

SENTINEL = -7.0   # float planes before a call writes them
TEXEL = 77        # rgb8 texels before a call writes them


@functools.lru_cache(maxsize=None)
def hip_runtime():
    """The HIP runtime the library is linked to, opened once, after rt.lib() has loaded it: the path
    this process has mapped, or the soname the library was built against."""
    rt.lib()
    name = "libamdhip64.so.7"
    with open("/proc/self/maps") as maps:
        for line in maps:
            if "/libamdhip64.so" in line:
                name = line.split(None, 5)[5].strip()
                break
    return C.CDLL(name)


def download(address, shape, dtype=np.float32):
    """The device array at `address` (the stream that wrote it is synchronised); None for a null address."""
    if not address:
        return None
    out = np.empty(shape, dtype=dtype)
    rc = hip_runtime().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(address), C.c_size_t(out.nbytes), C.c_int(2))
    assert rc == 0, f"hipMemcpy device to host of {out.nbytes} bytes: {rc}"
    return out


def read_planes(pv, w, h, table=abi.PREVIEW_PLANES, addresses=None):
    """A preview session's planes (rt_preview_planes) on the host: {name: array, or None where the mode
    keeps no such plane}; table / addresses: another record of w x h planes (rt_preview_output)."""
    pl = pv.planes() if addresses is None else addresses
    return {n: download(pl[n], (h, w, 3) if ch == 3 else (h, w), dt) for n, (ch, dt) in table.items()}


def filled(shape, value, dtype=None):
    """A tensor on cuda:0 with every element `value` (dtype: float32 if None)."""
    import torch
    return torch.full(tuple(shape), value, dtype=dtype or torch.float32, device="cuda:0")


def plane(w, h, ch, dtype=None):
    """A sentinel-filled device plane: (h, w, ch), or (h, w) for one channel."""
    return filled((h, w, ch) if ch > 1 else (h, w), SENTINEL, dtype)


class Outputs:
    """Sentinel-filled device images of a session call (rgb float32, rgb8 uint8; either may be
    absent) and, unless own_stream is False, a stream of their own made after a device synchronise."""

    def __init__(self, w, h, f32=True, u8=True, own_stream=True):
        import torch
        self.rgb = plane(w, h, 3) if f32 else None
        self.rgb8 = filled((h, w, 3), TEXEL, torch.uint8) if u8 else None
        self.stream = None
        if own_stream:
            torch.cuda.synchronize()
            self.stream = torch.cuda.Stream()

    def pointers(self):
        return tuple(t.data_ptr() if t is not None else None for t in (self.rgb, self.rgb8))

    def host(self):
        return tuple(t.cpu().numpy() if t is not None else None for t in (self.rgb, self.rgb8))

    def frame(self, pv, cam, seed):
        """rt_preview_frame_device into these images on their stream: (rgb, rgb8) on the host."""
        pv.frame(cam, seed, *self.pointers(), self.stream.cuda_stream)
        self.stream.synchronize()
        return self.host()

    def refine(self, pv, cam, seed, total, n):
        """rt_preview_refine_device into these images on their stream: (rgb, rgb8) on the host."""
        pv.refine(cam, seed, total, n, *self.pointers(), self.stream.cuda_stream)
        self.stream.synchronize()
        return self.host()
