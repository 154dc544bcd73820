"""TEST INFRASTRUCTURE: CPU restatement of a preview session with rt_preview_set_clip (include/rt_api.h;
DESIGN.md §4.17) in numpy float32: preview_ref.Session whose temporal stage is
temporal_clip_ref.accumulate while a clip record is set, and preview_ref's own frame otherwise.

    s = preview_clip_ref.Session(params)             # an rt_preview_params record
    s.set_clip(clip)                                 # an rt_temporal_clip_t record, or None: off
    r = s.frame(cur, camera)                         # as preview_ref.Session.frame; r["info"]: the clamp's

The clip takes effect from the next frame and keeps the history (s.prev). Under RT_PREVIEW_DEMODULATE
the window is taken over the illumination, which is what the temporal stage sees as its beauty.
"""
import denoise_var_ref
import preview_ref
import temporal_clip_ref
from preview_ref import DEMODULATE, FEEDBACK, GUIDES, NO_TEMPORAL, _f32, merge, split


class Session(preview_ref.Session):
    def __init__(self, params):
        super().__init__(params)
        self.clip = None

    def set_clip(self, clip):
        assert not self.p.flags & NO_TEMPORAL, "a session without a temporal stage takes no clip"
        self.clip = clip

    def frame(self, cur, camera):
        if self.clip is None:
            return dict(super().frame(cur, camera), info=None)
        p, fl = self.p, self.p.flags
        color, variance = _f32(cur["beauty"]), _f32(cur["variance"])
        if fl & DEMODULATE:
            color, variance = split(color, variance, cur["albedo"])
        tcur = dict(beauty=color, variance=variance, alpha=cur["alpha"], **{n: cur[n] for n in GUIDES})
        color, variance, history, reason, info = temporal_clip_ref.accumulate(tcur, self.prev, camera, self.prev_camera,
                                                                              p.temporal, self.clip)
        kw = dict(sigma_color=p.denoise.sigma_color, sigma_normal=p.denoise.sigma_normal,
                  sigma_depth=p.denoise.sigma_depth, sigma_albedo=p.denoise.sigma_albedo, var_floor=p.var_floor)
        guides = (cur["albedo"], cur["normal"], cur["depth"])
        filtered = denoise_var_ref.denoise(color, variance, *guides, levels=p.denoise.levels, **kw)[0]
        back_c, back_v = color, variance
        if fl & FEEDBACK:
            back_c, back_v, _ = denoise_var_ref.denoise(color, variance, *guides, levels=1, **kw)
        self.prev = dict(color=back_c, variance=back_v, history=history, **{n: cur[n] for n in GUIDES})
        self.prev_camera = camera
        out = merge(filtered, cur["albedo"] if fl & DEMODULATE else None)
        return dict(out=out, color=color, variance=variance, history=history, reason=reason, info=info)
