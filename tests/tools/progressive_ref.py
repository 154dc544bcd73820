"""TEST INFRASTRUCTURE: the CPU restatement of a progressive session (rt_progressive_*, DESIGN.md
§4.19), in numpy float32, line by line from the contract in include/rt_api.h. Its input is the
per-sample colours that tests/tools/moments_ref.render returns, (rendered rows, width, spp, 3): the
samples of the WHOLE frame, of which a session has folded a prefix.

    s = progressive_ref.Session(samples)
    s.step(4)
    est = s.resolve(tau=0.1)      # dict rgb, var, rgb8, noisy after s.done samples

The carried sum is the frame's own addition order carried across windows: per block of 4 samples
acc = acc + ((c0 + c1) + (c2 + c3)), then the spp % 4 tail one by one. The luminance moments
{L_0, m1, m2} are carried window by window too, sample by sample: d = L_s - L_0, m1 = m1 + d,
m2 = m2 + d d, and the variance is formed from them at the resolve (moments_ref.variance computes
the same quantity from a whole prefix at once; the tests compare the two).
"""
import numpy as np

import moments_ref

F = np.float32


def window(spp, done, n):
    """The Step rule: the samples a step of n takes, or ValueError where it is refused."""
    left = spp - done
    if n % 4 and n < left:
        raise ValueError("n_samples must be a multiple of 4 before the frame's end")
    return min(n, left)


def texel(c):
    """rgb8_texel: pow(c, 1 / 2.2f) in double, narrowed to float32, then (uint8)(255 c)."""
    g = np.float64(F(1) / F(2.2))
    t = F(255) * np.power(np.asarray(c, dtype=F).astype(np.float64), g).astype(F)
    assert t.dtype == F
    return t.astype(np.uint8)  # (truncation; every value is in [0, 255])


class Session:
    def __init__(self, samples):
        samples = np.asarray(samples)
        assert samples.dtype == F and samples.ndim == 4 and samples.shape[3] == 3
        self.samples = samples
        self.spp = samples.shape[2]
        assert self.spp >= 2
        self.done = 0
        self.acc = np.zeros(samples.shape[:2] + (3,), dtype=F)
        self.l0 = np.zeros(samples.shape[:2], dtype=F)
        self.m1 = np.zeros(samples.shape[:2], dtype=F)
        self.m2 = np.zeros(samples.shape[:2], dtype=F)

    def step(self, n):
        m = window(self.spp, self.done, n)
        c = self.samples
        blocks_end = self.spp & ~3  # samples [0, blocks_end) form blocks of 4
        s, end = self.done, self.done + m
        while s < min(end, blocks_end):
            self.acc = self.acc + ((c[:, :, s] + c[:, :, s + 1]) + (c[:, :, s + 2] + c[:, :, s + 3]))
            s += 4
        while s < end:
            self.acc = self.acc + c[:, :, s]
            s += 1
        for t in range(self.done, end):       # the moments: sequential, in sample order
            lum = moments_ref.luminance(c[:, :, t])
            if t == 0:
                self.l0 = lum                     # the frame's sample 0: d = 0
            d = lum - self.l0
            self.m1 = self.m1 + d
            self.m2 = self.m2 + d * d
        assert self.acc.dtype == F and self.m1.dtype == F and self.m2.dtype == F
        self.done = end
        return m

    def resolve(self, tau=None):
        d = self.done
        assert d >= 2
        rgb = self.acc / F(d)
        nf = F(d)
        mean = self.m1 / nf
        ex2 = self.m2 / nf
        var = np.fmax(F(0), ex2 - mean * mean) / F(d - 1)
        out = dict(rgb=rgb, var=var, rgb8=texel(rgb))
        if tau is not None:
            t2 = F(tau) * F(tau)
            lum = moments_ref.luminance(rgb)
            out["noisy"] = int(np.count_nonzero(var > t2 * (lum * lum)))
        assert rgb.dtype == F and var.dtype == F
        return out


def run(samples, windows, tau=None):
    """The estimates after each window of `windows` (sample counts): a list of resolve() dicts."""
    s = Session(samples)
    out = []
    for n in windows:
        s.step(n)
        out.append(s.resolve(tau))
    return out


def place(est, params, sentinel=None):
    """An estimate's planes laid out as `params` says (RT_FLAG_FULL_FRAME: rows at their global
    position, the others `sentinel`)."""
    from raytracinginoneweekend_amd import _abi as abi
    if not params.flags & abi.RT_FLAG_FULL_FRAME:
        return est
    st, off, rows = params.row_stride or 1, params.row_offset, est["rgb"].shape[0]
    out = dict(est)
    for name in ("rgb", "var", "rgb8"):
        a = est[name]
        full = np.full((params.height,) + a.shape[1:], sentinel[name], dtype=a.dtype)
        full[off:off + rows * st:st] = a
        out[name] = full
    return out
