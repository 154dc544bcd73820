"""The dealing order computed on the device (rt_options.tile_classes = 1, rt_tile_order_device;
DESIGN.md §4.13).

The contract is equality, not closeness: the device's kernels evaluate the host's expression tree
(csrc/rt_tiles.h), so permutations and counts are compared entry for entry with rt_tile_order's,
and frames bit for bit (uint32 views, zero mismatches) with the oracle's or with the frames of a
scene whose orders come from the host.
"""
import os
import sys

import numpy as np
import pytest

import golden_io as G
import oracle_binding as O
import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import camera_cases as CC  # noqa: E402
from support import assert_bits as _bits_equal, orbit_camera  # noqa: E402

pytestmark = pytest.mark.gpu


def orbit(w, h, i, mode=rt.REFERENCE):
    return orbit_camera(w, h, i, mode=mode)


def _same_order(ds, scene, cam, p, what):
    want, wl, ws = rt.tile_order(scene, p, cam)
    got, gl, gs = ds.tile_order(cam, p)
    print(what, "blocks", len(want), "lead", wl, "sky", ws, "| device lead", gl, "sky", gs)
    assert (gl, gs) == (wl, ws), what
    assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), what
    return len(want), wl, ws


# ---- 1. the classes equal the host's, exactly --------------------------------------------------
def test_camera_cases_get_the_hosts_order():
    """Every camera case at its own frame (64 x 40: 40 blocks, a partial wave; `natural` 37 x 19: no
    blocks; `share`: a row stride), among them frames that are all sky, frames without a sky tile,
    the subnormal directions and the lens wider than the scene."""
    scenes, seen = {}, {}
    for name in CC.NAMES:
        c = CC.case(name)
        key = (c.spheres.tobytes(), c.materials.tobytes())
        if key not in scenes:
            scenes[key] = rt.DeviceScene((c.spheres, c.materials))
        seen[name] = _same_order(scenes[key], (c.spheres, c.materials), c.camera, CC.params(name), name)
    for ds in scenes.values():
        assert ds.order_counts() == {"host_orders": 0, "device_orders": 0, "hits": 0}  # not a render's orders
        ds.close()
    nb, nl, ns = seen["up_clear"]
    assert nb == 40 and nl == 0 and ns == 40  # all sky, no lead
    assert seen["in_glass"][2] == 0 and seen["in_bubble"][2] == 0  # cameras inside glass: no sky
    assert seen["natural"][0] == 0
    assert 0 < seen["up_tilt"][1] and 0 < seen["up_tilt"][2]  # lead, middle and sky tiles in one frame


FRAMES = [(72, 40, {}), (64, 44, {}), (100, 64, {}), (200, 100, {}), (320, 176, {}),
          (256, 144, dict(row_offset=3, row_stride=4, num_rows=36))]


@pytest.fixture(scope="module")
def huge():
    s, m = G.scene("huge")
    ds = rt.DeviceScene((s, m))
    yield (s, m), ds
    ds.close()


@pytest.mark.parametrize("mode", [rt.REFERENCE, rt.CORRECTED])
def test_huge_scene_frames_get_the_hosts_order(huge, mode):
    """45 blocks; rows left over below the tiles (class 1, in their place); a width that is no
    multiple of 8 (the identity, zero counts); pixels not in whole blocks (no blocks); 880 blocks;
    an interleaved row share."""
    scene, ds = huge
    got = {}
    for W, H, rows in FRAMES:
        p = rt.make_params(W, H, 4, 64, 21, **rows)
        got[(W, H)] = _same_order(ds, scene, rt.Camera.default(W, H, mode), p, f"{W}x{H} {rows} camera {mode}")
    assert got[(72, 40)][0] == 45 and got[(64, 44)][0] == 44 and got[(320, 176)][0] == 880 and got[(256, 144)][0] == 144
    assert got[(100, 64)] == (100, 0, 0) and got[(200, 100)] == (0, 0, 0)
    if mode == rt.REFERENCE:
        assert got[(320, 176)][1] > 0 and got[(320, 176)][2] > 0


def test_config_3_frame_gets_the_hosts_order(huge):
    """1280 x 720: 14 400 blocks, 225 waves of tiles and 15 chunks of the partition."""
    scene, ds = huge
    W, H = 1280, 720
    for mode in (rt.REFERENCE, rt.CORRECTED):
        nb, nl, ns = _same_order(ds, scene, rt.Camera.default(W, H, mode), rt.make_params(W, H, 8, 64, 1), f"c3 camera {mode}")
        assert nb == 14400 and nl > 0
        if mode == rt.REFERENCE:
            assert ns > nb // 2  # most of config 3's frame is sky


# ---- 2. renders keep their bits ----------------------------------------------------------------
ORDER_CASES = [(320, 176, 12, {}, 0), (320, 176, 12, {}, 0), (256, 144, 8, dict(row_offset=3, row_stride=4, num_rows=36), 0),
               (192, 112, 8, {}, 1)]


@pytest.fixture(scope="module")
def order_case_refs():
    """The oracle's frames of ORDER_CASES, once for every test below."""
    s, m = G.scene("huge")
    refs = []
    for W, H, spp, rows, mode in ORDER_CASES:
        p = rt.make_params(W, H, spp, 64, 21, **rows)
        img, _ = O.render_f32(s, m, O.camera_default(W, H, mode), p)
        img.flags.writeable = False
        refs.append(img)
    return refs


def _render_cases(torch, scene):
    ds = rt.DeviceScene(scene)
    stream = torch.cuda.current_stream().cuda_stream
    outs, used = [], []
    for W, H, spp, rows, mode in ORDER_CASES:
        p = rt.make_params(W, H, spp, 64, 21, **rows)
        o = torch.empty((abi.rows_of(p), W, 3), dtype=torch.float32, device="cuda")
        ds.render(rt.Camera.default(W, H, mode), p, o.data_ptr(), stream)
        used.append(ds.usage())
        outs.append(o)
    torch.cuda.synchronize()
    counts = ds.order_counts()
    ds.close()
    return [o.cpu().numpy() for o in outs], used, counts


@pytest.mark.parametrize("order", ["classes", "sky_serial", "no_sky", "natural_order"])
def test_dealing_orders_from_the_device_keep_the_bits(order, opts, order_case_refs):
    """test_dealing_orders_keep_the_bits' four frames with the orders computed on the device: the
    oracle's bits, the host mode's class counts, and no order from the host."""
    torch = pytest.importorskip("torch")
    diag = {"classes": {}, "sky_serial": dict(sky_serial=True), "no_sky": dict(no_sky=True),
            "natural_order": dict(natural_order=True)}[order]
    scene = G.scene("huge")
    opts.set(deep_min_items=0, **diag)
    _, host_used, host_counts = _render_cases(torch, scene)
    opts.set(tile_classes=1)
    imgs, used, counts = _render_cases(torch, scene)
    for case, img, want, u, hu in zip(ORDER_CASES, imgs, order_case_refs, used, host_used):
        _bits_equal(img, want, f"{order} {case}")
        assert (u["lead_tiles"], u["sky_tiles"]) == (hu["lead_tiles"], hu["sky_tiles"]), (case, u, hu)
        if order != "natural_order" and case[4] == 0:
            assert u["lead_tiles"] > 0, u
    # three distinct (camera, rows) and the second frame a repeat of the first; none without classes
    n = 0 if order == "natural_order" else 3
    assert counts == {"host_orders": 0, "device_orders": n, "hits": n // 3}, counts
    assert host_counts == {"host_orders": n, "device_orders": 0, "hits": n // 3}, host_counts
    assert used[0]["split_passes"] == 1, used[0]


def test_device_orders_of_other_cluster_sizes_keep_the_bits(opts, order_case_refs):
    """cluster_size = 32: other boxes, other classes, the same frames (rt_tile_order has the default
    cluster size only, so the frames are the check)."""
    torch = pytest.importorskip("torch")
    opts.set(deep_min_items=0, tile_classes=1, cluster_size=32)
    imgs, used, counts = _render_cases(torch, G.scene("huge"))
    for case, img, want in zip(ORDER_CASES, imgs, order_case_refs):
        _bits_equal(img, want, f"cluster_size 32 {case}")
    assert counts == {"host_orders": 0, "device_orders": 3, "hits": 1}, counts
    assert used[0]["lead_tiles"] > 0


# ---- 3. a moving camera ------------------------------------------------------------------------
def _orbit_frames(torch, scene, cams, p):
    ds = rt.DeviceScene(scene)
    stream = torch.cuda.current_stream().cuda_stream
    outs = [torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda") for _ in cams]
    for cam, o in zip(cams, outs):  # back to back: no synchronisation of the caller's between the frames
        ds.render(cam, p, o.data_ptr(), stream)
    torch.cuda.synchronize()
    counts = ds.order_counts()
    ds.close()
    return [o.cpu().numpy() for o in outs], counts


def test_a_camera_that_moves_every_frame(opts):
    """12 cameras of the orbit, more than the 8 orders a scene keeps, then the first again, enqueued
    back to back: every frame equals the host-mode scene's. The pool is least-recently-used and
    every camera is used once, so the first camera's order has left when it returns: 13 orders from
    the device, no hit, none from the host; the permutation slots were written again while earlier
    frames could still read them."""
    torch = pytest.importorskip("torch")
    W, H, spp = 192, 96, 4
    scene = G.scene("huge")
    p = rt.make_params(W, H, spp, 64, 9)
    cams = [orbit(W, H, i) for i in range(12)]
    cams.append(cams[0])
    opts.set(tile_classes=0)
    want, host_counts = _orbit_frames(torch, scene, cams, p)
    opts.set(tile_classes=1)
    got, counts = _orbit_frames(torch, scene, cams, p)
    for i, (a, b) in enumerate(zip(got, want)):
        _bits_equal(a, b, f"orbit frame {i}")
    _bits_equal(got[12], got[0], "the first camera again")
    assert host_counts == {"host_orders": 13, "device_orders": 0, "hits": 0}, host_counts
    assert counts == {"host_orders": 0, "device_orders": 13, "hits": 0}, counts


# ---- 4. the preview session --------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, abi.RT_PREVIEW_NO_TEMPORAL])
def test_preview_session_on_a_device_mode_scene(flags):
    """10 orbit frames at 64 x 36, 4 spp: a session on a scene with tile_classes = 1 writes the rgb
    and rgb8 of one on a host-mode scene, and each frame computes one order (the render's), which
    its feature-buffer call finds cached."""
    torch = pytest.importorskip("torch")
    W, H, n = 64, 36, 10
    scene = rt.huge_scene_arrays(1234)
    frames = {}
    for tc in (0, 1):
        ds = rt.DeviceScene(scene, options=rt.options(tile_classes=tc))
        pv = ds.preview(rt.preview_params(W, H, 4, flags=flags, max_depth=8))
        rgb = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda")
        rgb8 = torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        out, counts = [], []
        for i in range(n):
            pv.frame(orbit(W, H, i, rt.CORRECTED), 1 + i, rgb.data_ptr(), rgb8.data_ptr(), stream.cuda_stream)
            counts.append(ds.order_counts())
            stream.synchronize()
            out.append((rgb.cpu().numpy(), rgb8.cpu().numpy()))
        pv.close()
        ds.close()
        frames[tc] = out
        side = "device_orders" if tc else "host_orders"
        for i, c in enumerate(counts):
            assert c == {"host_orders": 0, "device_orders": 0, "hits": i + 1, side: i + 1}, (tc, i, c)
    for i, ((a, a8), (b, b8)) in enumerate(zip(frames[1], frames[0])):
        _bits_equal(a, b, f"preview frame {i} rgb")
        _bits_equal(a8, b8, f"preview frame {i} rgb8")


# ---- 5. rt_tile_order_device's bounds ----------------------------------------------------------
def test_tile_order_device_capacity(huge):
    """A buffer too small is RT_ERR_CAPACITY with the counts set and nothing written, neither in
    the buffer nor behind it; one of the exact size is filled and the words behind it stay."""
    import ctypes as C
    torch = pytest.importorskip("torch")
    scene, ds = huge
    W, H = 72, 40
    cam, p = rt.Camera.default(W, H), rt.make_params(W, H, 1)
    want, wl, ws = rt.tile_order(scene, p, cam)
    n, guard = len(want), 0x5AFEC0DE
    assert n == 45
    L = rt.lib()
    for cap in (1, n - 1, n):
        buf = torch.full((n + 64,), guard, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        nb, nl, ns = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        rc = L.rt_tile_order_device(ds.handle, C.byref(cam.c), C.byref(p), C.c_void_p(buf.data_ptr()), cap, C.byref(nb),
                                    C.byref(nl), C.byref(ns), None)
        words = buf.cpu().numpy().view(np.uint32)
        assert (nb.value, nl.value, ns.value) == (n, wl, ws), cap
        if cap < n:
            assert rc == abi.RT_ERR_CAPACITY and b"too small" in L.rt_last_error(), cap
            assert (words == guard).all(), cap
        else:
            assert rc == abi.RT_OK
            assert np.array_equal(words[:n], want) and (words[n:] == guard).all()
