"""Every kernel that stores rgb8 texels, against the texel's table (tests/tools/texel_ref.py,
tests/golden/texel_steps.json: the 255 words at which the contract's texel steps over its domain, the
floats with words 0 .. 0x3f811b5e).

* epilogue_rgb8_kernel (rt_epilogue_rgb8_device) on EVERY float of the domain, compared on the device:
  this measures the device's double pow against the correctly rounded one on all 2^30 inputs.
* preview_merge (rt_preview_merge_device) and progressive_resolve (a resolve-only step of a progressive
  session) on the floats within 8 of every step and the domain's edges: a rendered frame lands that
  close to a step in well under 1 of 10 000 values, so only placed values see a texel function that is
  wrong by an ulp.
adaptive_resolve has no checkpoint to inject into; it stays on its exact comparison over rendered
frames (tests/test_adaptive_gpu.py).

Tolerance: none. Every texel equals the table's.
"""
import os
import sys
import time

import numpy as np
import pytest

import golden_io as G
import raytracinginoneweekend_amd as rt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import texel_ref as T  # noqa: E402
from device_io import SENTINEL, TEXEL, filled  # noqa: E402
from support import words  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 3 << 24      # values per call of the sweep: 2^24 pixels
GUARD = 256          # sentinel bytes kept behind every texel plane
PARTS = 1            # the sweep's parametrized ranges (chunks dealt round the parts in order)
W = 67               # the window images' width: no multiple of preview_merge's 64 x 4 workgroup


def _chunks():
    return [(a, min(a + CHUNK, T.LAST + 1)) for a in range(0, T.LAST + 1, CHUNK)]


# ---- epilogue_rgb8_kernel: every float ----------------------------------------------------------------
@pytest.mark.parametrize("part", range(PARTS))
def test_epilogue_texel_on_every_float_of_the_domain(part):
    """Words 0 .. LAST in chunks of 3 * 2^24 values (the last ragged: padded to whole pixels with the
    domain's last float), made on the device, through rt_epilogue_rgb8_device on a stream of its own into
    a sentinel-filled plane; expected: torch.bucketize over the 255 step words. Zero mismatches, and
    the bytes behind the plane keep the sentinel."""
    import torch
    chunks = _chunks()
    assert len(chunks) == 22 and chunks[-1][1] - chunks[-1][0] == (T.LAST + 1) - 21 * CHUNK
    mine = chunks[part * len(chunks) // PARTS:(part + 1) * len(chunks) // PARTS]
    steps = torch.tensor(T.steps().astype(np.int32), dtype=torch.int32, device="cuda:0")
    st = torch.cuda.Stream()
    bad_total, first, checked = 0, [], 0
    t0 = time.perf_counter()
    with torch.cuda.stream(st):
        for a, b in mine:
            n_px = (b - a + 2) // 3
            bits = torch.arange(a, a + 3 * n_px, dtype=torch.int32, device="cuda:0").clamp_(max=T.LAST)
            out = filled((3 * n_px + GUARD,), TEXEL, torch.uint8)
            rt.epilogue_rgb8_device(bits.view(torch.float32).data_ptr(), out.data_ptr(), n_px, st.cuda_stream)
            want = torch.bucketize(bits, steps, right=True).to(torch.uint8)
            bad = out[:3 * n_px] != want
            n_bad = int(bad.sum())
            assert bool((out[3 * n_px:] == TEXEL).all()), f"chunk {a:#010x}: bytes behind the plane were written"
            if n_bad and len(first) < 8:
                for i in torch.nonzero(bad).reshape(-1)[:8 - len(first)].tolist():
                    first.append(f"{int(bits[i]):#010x} got {int(out[i])} want {int(want[i])}")
            bad_total += n_bad
            checked += b - a
            del bits, out, want, bad
    st.synchronize()
    dt = time.perf_counter() - t0
    print(f"epilogue_rgb8_kernel, words {mine[0][0]:#010x} .. {mine[-1][1] - 1:#010x}: {bad_total} of {checked} "
          f"texels differ from the table, {dt:.2f} s{'; first ' + str(first) if first else ''}")
    assert bad_total == 0, f"{bad_total} of {checked} texels differ from the table, first {first}"


def test_epilogue_windows_negative_zero_and_the_plane_end():
    """One more call on the window floats, -0.0 among them: -0.0 gives 0, every texel is the table's, and
    the bytes past 3 * n_pixels keep the sentinel (the values past a whole pixel are not converted)."""
    import torch
    f = T.windows(8)
    n_px = (f.size - 1) // 3      # the floats past the last converted pixel (one at least) stay unconverted
    assert words(f)[-1] == 0x80000000
    f = np.concatenate([f[-1:], f[:-1]])   # -0.0 first, inside the converted pixels
    src = torch.from_numpy(f).to("cuda:0")
    out = filled((f.size + GUARD,), TEXEL, torch.uint8)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.default_stream())
    rt.epilogue_rgb8_device(src.data_ptr(), out.data_ptr(), n_px, st.cuda_stream)
    st.synchronize()
    got = out.cpu().numpy()
    assert got[0] == 0
    T.assert_texels(got[:3 * n_px], f[:3 * n_px], "epilogue on windows(8)")
    assert (got[3 * n_px:] == TEXEL).all(), "bytes past 3 * n_pixels were written"


# ---- the window image ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def window_image():
    """windows(8) as a 67-wide rgb image, padded with step floats: read-only (h, 67, 3) float32."""
    f = T.windows(8)
    h = -(-f.size // (3 * W))
    pad = np.resize(T.steps().view(np.float32), 3 * W * h - f.size)
    img = np.concatenate([f, pad]).reshape(h, W, 3)
    assert h % 4 != 0 and np.isin(words(f), words(img)).all()
    img.setflags(write=False)
    return img


def _merge(filtered, albedo, f32, u8):
    """rt_preview_merge_device of a host plane (albedo: one value for the whole plane, or None) into
    sentinel-filled planes, of which only those asked for are passed: both planes, read back."""
    import torch
    h, w, _ = filtered.shape
    src = torch.from_numpy(np.ascontiguousarray(filtered)).to("cuda:0")
    alb = None if albedo is None else filled((h, w, 3), albedo)
    rgb = filled((h, w, 3), SENTINEL)
    rgb8 = filled((h * w * 3 + GUARD,), TEXEL, torch.uint8)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    rt.preview_merge_device(w, h, src.data_ptr(), alb.data_ptr() if alb is not None else None,
                            rgb.data_ptr() if f32 else None, rgb8.data_ptr() if u8 else None, st.cuda_stream)
    st.synchronize()
    return rgb.cpu().numpy(), rgb8.cpu().numpy()


@pytest.mark.parametrize("albedo,scale", [(None, 1.0), (1.0, 1.0), (0.5, 2.0)])
@pytest.mark.parametrize("outputs", ["u8", "f32+u8", "f32"])
def test_preview_merge_texels_on_the_windows(window_image, albedo, scale, outputs):
    """preview_merge's six instantiations on the window floats: filtered = scale * c with albedo 1 / scale
    (the product is c exactly, subnormals included), so the f32 output's words are the window floats and
    the texels are the table's of them; an output not asked for keeps its sentinel, as do the bytes
    behind the texel plane."""
    img = window_image
    filtered = img * np.float32(scale)
    assert filtered.dtype == np.float32 and np.array_equal(words(filtered * np.float32(1 / scale)), words(img))
    f32, u8 = "f32" in outputs, "u8" in outputs
    rgb, rgb8 = _merge(filtered, albedo, f32, u8)
    what = f"preview_merge albedo {albedo} outputs {outputs}"
    n = img.size
    assert (rgb8[n:] == TEXEL).all(), f"{what}: bytes behind the texel plane were written"
    if f32:
        bad = int(np.count_nonzero(words(rgb) != words(img)))
        assert bad == 0, f"{what}: {bad} of {n} f32 words are not the window floats"
    else:
        assert (rgb == np.float32(SENTINEL)).all(), f"{what}: the f32 plane was written"
    if u8:
        T.assert_texels(rgb8[:n], rgb if f32 else img, what)
    else:
        assert (rgb8 == TEXEL).all(), f"{what}: the texel plane was written"


# ---- progressive_resolve ------------------------------------------------------------------------------
HEADER_BYTES = 128   # a checkpoint's head: magic, version, layout, rt_params, rt_camera, n_pixels, done, reserved


def test_progressive_resolve_texels_on_the_windows():
    """progressive_resolve on the window floats, injected through a checkpoint. A checkpoint is opaque by
    contract (include/rt_api.h); THIS TEST IS THE ONE PLACE THAT READS ITS LAYOUT: a head of 128 bytes,
    then the sums plane and the moments plane, 12 * n_pixels bytes each (rt_host_post.cpp,
    rt_progressive_save / rt_progressive_load). A 67 x 19 session on the simple scene takes 4 samples
    and is saved; the sums plane is overwritten with 4 c (exact, subnormals included; 4 c / 4 is c), the
    blob loaded, and a resolve-only step (n_samples = 0) stores rgb and rgb8. The plane holds 3819 values,
    the windows 4340: two rounds, the second padded with step floats. The sums lie in dealing order, so
    the test compares the multiset of rgb words with the injected floats, then the texels with the
    table's of the rgb plane it read back."""
    import torch
    w, h, spp = W, 19, 8
    n_px = w * h
    s, m = G.scene("simple")
    p, cam = rt.make_params(w, h, spp, 64, 7), rt.Camera.default(w, h)
    f = T.windows(8)
    rounds = -(-f.size // (3 * n_px))
    vals = np.concatenate([f, np.resize(T.steps().view(np.float32), rounds * 3 * n_px - f.size)]).reshape(rounds, 3 * n_px)
    ds = rt.DeviceScene((s, m), device=0)
    try:
        pg = ds.progressive(cam, p)
        info = pg.info()
        head = info["state_bytes"] - 24 * n_px
        assert info["n_pixels"] == n_px and head == HEADER_BYTES, \
            (f"the checkpoint's layout changed: state_bytes - 24 * n_pixels = {head}, this test expects a head of "
             f"{HEADER_BYTES} bytes before the sums and moments planes; read rt_progressive_save and mend the test")
        pg.step(4)
        blob = bytearray(pg.save())
        assert len(blob) == info["state_bytes"]
        st = torch.cuda.Stream()
        for k in range(rounds):
            c = vals[k]
            sums = c * np.float32(4)
            assert sums.dtype == np.float32 and np.array_equal(words(sums / np.float32(4)), words(c))
            blob[HEADER_BYTES:HEADER_BYTES + 12 * n_px] = sums.tobytes()
            pg.load(bytes(blob))
            rgb = filled((h, w, 3), SENTINEL)
            rgb8 = filled((n_px * 3 + GUARD,), TEXEL, torch.uint8)
            torch.cuda.synchronize()
            pg.step(0, rgb_ptr=rgb.data_ptr(), rgb8_ptr=rgb8.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            assert pg.info()["done"] == 4
            got, got8 = rgb.cpu().numpy(), rgb8.cpu().numpy()
            what = f"progressive_resolve round {k}"
            assert np.array_equal(np.sort(words(got).reshape(-1)), np.sort(words(c))), \
                f"{what}: the rgb plane's words are not the injected floats"
            assert (got8[3 * n_px:] == TEXEL).all(), f"{what}: bytes behind the texel plane were written"
            T.assert_texels(got8[:3 * n_px], got, what)
        pg.close()
    finally:
        ds.close()
