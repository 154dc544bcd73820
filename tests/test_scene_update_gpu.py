"""rt_scene_update on the GPU: an updated scene against a scene freshly created
from the same records, bit for bit, in every call's output; the epochs and the two sphere tables; what
an identical update costs; refusals.

The simple scene's pair of records is tests/tools/motion_cases.py's, whose CPU test proves that the
trap windows and the dealing order differ between A and B, so the equality here rests on re-derived
tables. Sizes 64 x 40 (whole 64-pixel blocks: a classified order) and 48 x 27 (the natural order).
"""
import os
import sys

import numpy as np
import pytest

import raytracinginoneweekend_amd as rt
from raytracinginoneweekend_amd import _abi as abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from motion_cases import huge_a_b, huge_far_a_b, records_a_b  # noqa: E402
from device_io import download  # noqa: E402
from support import assert_all_bits, assert_bits, words as u32  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SPP = 4
SIZES = ((64, 40), (48, 27))
AOV = tuple(abi.AOV_PLANES)


def everything(ds, w, h, brute=True):
    """Every output of every call on a device scene for one camera: a dict name -> array."""
    import torch
    cam = rt.Camera.default(w, h, rt.CORRECTED)
    p = rt.make_params(w, h, SPP, 16, 5)
    dev = "cuda:0"
    st = torch.cuda.Stream()
    out = {}
    rgb, rgb2, var = (torch.full(s, -7.0, dtype=torch.float32, device=dev) for s in ((h, w, 3), (h, w, 3), (h, w)))
    planes = {n: torch.full((h, w, 3) if ch == 3 else (h, w), -7.0 if dt == np.float32 else 7,
                            dtype=torch.float32 if dt == np.float32 else torch.int32, device=dev)
              for n, (ch, dt, _) in abi.AOV_PLANES.items()}
    torch.cuda.synchronize()
    ds.render(cam, p, rgb.data_ptr(), st.cuda_stream)
    st.synchronize()
    out["render"] = rgb.cpu().numpy()
    if brute:
        pb = rt.make_params(w, h, SPP, 16, 5, brute_force=True)
        rgb.fill_(-7.0)
        torch.cuda.synchronize()
        ds.render(cam, pb, rgb.data_ptr(), st.cuda_stream)
        st.synchronize()
        out["render brute force"] = rgb.cpu().numpy()
    ds.render_var(cam, p, rgb2.data_ptr(), var.data_ptr(), st.cuda_stream)
    ds.render_aov(cam, p, {n: a.data_ptr() for n, a in planes.items()}, 0, st.cuda_stream)
    st.synchronize()
    out["render_var beauty"], out["render_var variance"] = rgb2.cpu().numpy(), var.cpu().numpy()
    for n, a in planes.items():
        out["aov " + n] = a.cpu().numpy()
    perm, n_lead, n_sky = ds.tile_order(cam, p, st.cuda_stream)
    out["tile_order perm"], out["tile_order counts"] = perm, np.array([n_lead, n_sky], dtype=np.uint32)
    usage = ds.usage()
    out["usage"] = np.array([usage["lead_tiles"], usage["sky_tiles"], usage["device_bytes"] - usage["workspace_bytes"]],
                            dtype=np.uint32)  # (4-byte words: the comparer takes no others)
    return out


def assert_equal_outputs(got, want, what):
    assert sorted(got) == sorted(want)
    assert_all_bits(got, want, what)
    for n in want:
        assert not (got[n].dtype == np.float32 and (got[n] == -7.0).any()), f"{what}: {n} holds a sentinel"


PAIRS = {"simple": records_a_b, "huge": huge_a_b, "huge-far": huge_far_a_b}


# ---- 1, 2: update equals create, and back -----------------------------------------------------------------
@pytest.mark.parametrize("tile_classes", [0, 1])
@pytest.mark.parametrize("which", sorted(PAIRS))
def test_update_equals_create_and_back(which, tile_classes):
    A, B = PAIRS[which]()
    opt = rt.options(tile_classes=tile_classes)
    sc = rt.DeviceScene(A, options=opt)
    fresh = {r: rt.DeviceScene(rec, options=opt) for r, rec in (("A", A), ("B", B))}
    for w, h in SIZES:
        before = everything(sc, w, h)                   # an order is cached, the workspaces exist
        assert_equal_outputs(before, everything(fresh["A"], w, h), f"{which} {w}x{h} before the update")
        sc.update(B)
        assert_equal_outputs(everything(sc, w, h), everything(fresh["B"], w, h), f"{which} {w}x{h} updated to B")
        counts = sc.order_counts()
        sc.update(A)
        assert_equal_outputs(everything(sc, w, h, brute=False), {k: v for k, v in before.items() if "brute" not in k},
                             f"{which} {w}x{h} back to A")
        after = sc.order_counts()
        # back at A the order was computed again: the update had dropped the cache. (The simple scene has
        # no clusters: its passes keep the natural order and no order is ever computed or cached.)
        computed = after["host_orders"] + after["device_orders"] - counts["host_orders"] - counts["device_orders"]
        assert computed >= 1 if which != "simple" else sum(after.values()) == 0, (counts, after)
    assert sc.motion()["geometry_epoch"] == 2 * len(SIZES) and sc.motion()["appearance_epoch"] == 0
    for d in (sc, *fresh.values()):
        d.close()


def test_the_update_changed_the_picture():
    """A and B render different pictures, and the far pair different orders: equality above is not vacuous."""
    A, B = records_a_b()
    a, b = (everything(rt.DeviceScene(r), 64, 40, brute=False) for r in (A, B))
    assert (u32(a["render"]) != u32(b["render"])).sum() > 100
    assert (a["aov sphere_id"] != b["aov sphere_id"]).sum() > 10
    A, B = huge_far_a_b()
    a, b = (everything(rt.DeviceScene(r), 64, 40, brute=False) for r in (A, B))
    assert not np.array_equal(a["tile_order perm"], b["tile_order perm"]) or \
        not np.array_equal(a["tile_order counts"], b["tile_order counts"])
    assert not np.array_equal(a["usage"][:2], b["usage"][:2])      # the renders' own lead tiles differ


# ---- 3: an identical update is free ---------------------------------------------------------------------
def test_identical_update_is_free():
    import torch
    A, _ = huge_a_b()
    sc = rt.DeviceScene(A)
    w, h = 64, 40
    cam, p = rt.Camera.default(w, h, rt.CORRECTED), rt.make_params(w, h, SPP, 16, 5)
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    sc.render(cam, p, rgb.data_ptr())
    torch.cuda.synchronize()
    first, c0, m0 = rgb.cpu().numpy(), sc.order_counts(), sc.motion()
    sc.update((A[0].copy(), A[1].copy()))
    m1 = sc.motion()
    assert (m1["geometry_epoch"], m1["appearance_epoch"]) == (m0["geometry_epoch"], m0["appearance_epoch"]) == (0, 0)
    assert (m1["centres"], m1["prev_centres"]) == (m0["centres"], m0["prev_centres"])
    sc.render(cam, p, rgb.data_ptr())
    torch.cuda.synchronize()
    c1 = sc.order_counts()
    assert c1["hits"] == c0["hits"] + 1 and c1["host_orders"] == c0["host_orders"] and c1["device_orders"] == c0["device_orders"]
    assert_bits(rgb.cpu().numpy(), first)
    sc.close()


# ---- 4: epochs and tables ----------------------------------------------------------------------------------
def test_epochs_and_tables():
    (s, m), _ = records_a_b()
    sc = rt.DeviceScene((s, m))
    usage_bytes = sc.usage()["device_bytes"]
    m0 = sc.motion()
    assert m0["n_spheres"] == 5 and m0["centres"] and m0["prev_centres"] and m0["centres"] != m0["prev_centres"]
    t0 = rt.sphere_table((s, m))
    assert np.array_equal(u32(download(m0["centres"], (5, 4))), u32(t0)) and np.array_equal(u32(download(m0["prev_centres"], (5, 4))), u32(t0))
    moved = s.copy()
    moved["center"][2, 2] = F(0.25)
    sc.update((moved, m))                                   # geometry only
    m1 = sc.motion()
    assert (m1["geometry_epoch"], m1["appearance_epoch"]) == (1, 0)
    assert_bits(download(m1["centres"], (5, 4)), rt.sphere_table((moved, m)))
    assert_bits(download(m1["prev_centres"], (5, 4)), t0)
    painted = m.copy()
    painted["albedo"][1, 0] = F(0.25)
    sc.update((moved, painted))                             # albedo only
    m2 = sc.motion()
    assert (m2["geometry_epoch"], m2["appearance_epoch"]) == (1, 1)
    # the same flattened records through other material indices: nothing changed
    more = np.concatenate([painted, painted[:1]])
    again = moved.copy()
    again["material"][0] = len(painted)
    sc.update((again, more))
    m3 = sc.motion()
    assert (m3["geometry_epoch"], m3["appearance_epoch"]) == (1, 1)
    resized = moved.copy()
    resized["radius"][2] = F(0.5)
    sc.update((resized, m))                                 # both: a radius, and the albedo back
    m4 = sc.motion()
    assert (m4["geometry_epoch"], m4["appearance_epoch"]) == (2, 2)
    assert_bits(download(m4["prev_centres"], (5, 4)), rt.sphere_table((moved, m)))
    assert sc.usage()["device_bytes"] == usage_bytes
    sc.close()


# ---- 5: refusals ------------------------------------------------------------------------------------------
def test_refused_updates_leave_the_scene_as_it_was():
    A, B = records_a_b()
    sc = rt.DeviceScene(A)
    before = everything(sc, 64, 40, brute=False)
    with pytest.raises(rt.RtError) as e:
        sc.update((B[0][:4], B[1]))
    assert e.value.status == abi.RT_ERR_INVALID and "n_spheres" in str(e.value)
    bad = B[0].copy()
    bad["material"][3] = 17
    with pytest.raises(rt.RtError) as e:
        sc.update((bad, B[1]))
    assert e.value.status == abi.RT_ERR_INVALID and "material index" in str(e.value)
    kind = B[1].copy()
    kind["kind"][0] = 9
    with pytest.raises(rt.RtError) as e:
        sc.update((B[0], kind))
    assert e.value.status == abi.RT_ERR_INVALID and "kind" in str(e.value)
    assert sc.motion()["geometry_epoch"] == 0
    assert_equal_outputs(everything(sc, 64, 40, brute=False), before, "after the refusals")
    sc.close()
