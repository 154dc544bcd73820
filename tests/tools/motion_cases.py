"""TEST INFRASTRUCTURE: the pairs of scene records the moving-sphere tests share."""
import numpy as np

import raytracinginoneweekend_amd as rt

F = np.float32


def records_a_b():
    """A: the simple scene. B: its glass sphere (index 3) alone moved from (-2, 1, 0) to (-4.5, 1.5, 0),
    out of its bubble and off the ground. The move the issue proposed (spheres 3 and 4 together to
    x = -1.05) changes neither table: a glass ball with a bubble inside is never isolated, so it has
    no trap window before or after, and the tile order at 64x40 stayed the same. This one gives
    sphere 3 a window it did not have and another dealing order."""
    s, m = rt.simple_scene_arrays()
    b = s.copy()
    b["center"][3] = (F(-4.5), F(1.5), F(0.0))
    return (s, m), (b, m)


def huge_a_b():
    """A: the huge scene (seed 1234). B: three of its small spheres moved by 0.3: indices 12, 13 and 15,
    isolated glass balls whose trap windows the move changes (the windows' margins depend on the centre)."""
    s, m = rt.huge_scene_arrays(1234)
    b = s.copy()
    for i, d in ((12, (0.3, 0.0, 0.0)), (13, (0.0, 0.0, 0.3)), (15, (-0.3, 0.0, 0.0))):
        assert b["radius"][i] == F(0.2)
        b["center"][i] = b["center"][i] + np.array(d, dtype=F)
    return (s, m), (b, m)


def huge_far_a_b():
    """A: the huge scene. B: the same three glass balls carried by (8, 4, 8), up and across the scene. A
    move of 0.3 changes the trap windows but no tile's class at 64 x 40 (no such move of any small sphere
    does: the tiles are coarse there), and the simple scene has no clusters, so a device scene of it deals
    in the natural order and caches no order at all. This move changes both the windows and, under the
    default corrected camera, the dealing order (32 lead tiles become 40)."""
    (s, m), _ = huge_a_b()
    b = s.copy()
    for i in (12, 13, 15):
        b["center"][i] = b["center"][i] + np.array((8.0, 4.0, 8.0), dtype=F)
    return (s, m), (b, m)
