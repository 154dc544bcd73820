"""TEST INFRASTRUCTURE: ctypes binding of tests/device/librt_probe.so (tests/device/rt_probe.hip:
one kernel per device function of rt_trace.h). The library is built by `make -C csrc` with the
product's flags; if it is missing, or older than one of its sources (an edited rt_trace.h must not be
tested through the previous build), `make -C csrc probe` runs, once per process and under a lock that
threads and processes share, and a failure of that is an error.

    out = probe.run("sqrt_scaled", [x], n_out=1)          # (n_out, n) uint32, on cuda:0
    probe.exact_by_reciprocal(1280.0), probe.make_udiv(1280)  # the host's checks, no GPU

Inputs are 32-bit planes of one length n (a multiple of 64: the kernels run whole waves); 64-bit
values go as two planes, low word first (split64 / join64). Outputs start as SENTINEL.
"""
import ctypes as C
import fcntl
import glob
import os
import subprocess
import threading

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(REPO, "tests", "device", "librt_probe.so")
SENTINEL = 0xA5A5A5A5
PROBES = ("sqrt_scaled", "ray_div", "roots", "div3", "div_const", "sphere_key", "in_range", "min16_key",
          "pcg_stream", "canonical", "unit_sphere", "refract", "normalize", "schlick_x", "udiv")
CSRC = os.path.join(REPO, "raytracinginoneweekend_amd", "csrc")
_lib = None
_lock = threading.Lock()


def stale():
    """make's question (is the library missing, or older than a source of its rule), asked of the sources
    themselves, so that a built tree that travels without its object files is not compiled again."""
    if not os.path.exists(PATH):
        return True
    srcs = [os.path.join(REPO, "tests", "device", "rt_probe.hip"), os.path.join(REPO, "include", "rt_api.h"),
            os.path.join(CSRC, "rt_host_build.cpp")] + glob.glob(os.path.join(CSRC, "*.h"))
    return max(os.path.getmtime(s) for s in srcs) > os.path.getmtime(PATH)


def build_if_stale():
    fd = os.open(os.path.dirname(PATH), os.O_RDONLY)    # the directory itself is the processes' lock
    try:
        fcntl.flock(fd, fcntl.LOCK_EX)
        if stale():
            subprocess.run(["make", "-C", CSRC, "probe"], check=True)
    finally:
        os.close(fd)


def lib():
    global _lib
    with _lock:
        if _lib is None:
            build_if_stale()
            L = C.CDLL(PATH)
            for name in PROBES:
                f = getattr(L, "rt_probe_" + name)
                f.restype = C.c_int
                f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
            L.rt_probe_exact_by_reciprocal.restype = C.c_int
            L.rt_probe_exact_by_reciprocal.argtypes = [C.c_float]
            L.rt_probe_make_udiv.restype = None
            L.rt_probe_make_udiv.argtypes = [C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
            _lib = L
        return _lib


def words(a):
    """A plane as uint32 words: float32 by its bits, bool as 0 / 1."""
    a = np.asarray(a)
    if a.dtype == np.bool_:
        return a.astype(np.uint32)
    assert a.dtype in (np.uint32, np.float32, np.int32), a.dtype
    return np.ascontiguousarray(a).view(np.uint32)


def split64(a):
    a = np.asarray(a, dtype=np.uint64)
    return [(a & np.uint64(0xFFFFFFFF)).astype(np.uint32), (a >> np.uint64(32)).astype(np.uint32)]


def join64(lo, hi):
    return (np.asarray(hi).astype(np.uint64) << np.uint64(32)) | np.asarray(lo).astype(np.uint64)


def run(name, planes, n_out, arg=0):
    """Launch probe `name` on the planes; returns its n_out output planes as (n_out, n) uint32."""
    import torch
    assert name in PROBES, name
    ins = np.stack([words(p) for p in planes])
    n = ins.shape[1]
    assert n > 0 and n % 64 == 0, f"{name}: {n} lanes are not whole waves"
    d_in = torch.from_numpy(ins.view(np.int32)).to("cuda:0")
    d_out = torch.full((n_out, n), int(np.uint32(SENTINEL).view(np.int32)), dtype=torch.int32, device="cuda:0")
    rc = getattr(lib(), "rt_probe_" + name)(d_in.data_ptr(), d_out.data_ptr(), n, arg,
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"rt_probe_{name}: HIP error {rc}"
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32)


def exact_by_reciprocal(b):
    return bool(lib().rt_probe_exact_by_reciprocal(float(b)))


def make_udiv(d):
    m, s1, s2 = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().rt_probe_make_udiv(int(d), C.byref(m), C.byref(s1), C.byref(s2))
    return m.value, s1.value, s2.value
