#!/usr/bin/env python3
"""Records the cut of a frame (streams, workspaces, pass sizes, pairs, splits, tile classes) as
rt_scene_usage_get reports it after a render, over a list of small frames and option sets, into
tests/golden/plan_usage.json. tests/test_plan_gpu.py replays the cases of that file through
run_case() below and requires the same fields: run this at the commit whose plans are the record,
before a change to the pass planning (rt_plan.cpp) or to the stages of render_device_impl.

Every case runs on a fresh scene with render_streams set explicitly (never auto). "lone": one frame
and a synchronise (its first pass is issued alone by construction). "in_flight": two frames under
the in_flight diagnostic option (every pass takes the in-flight path whatever the device's timing).
Each case is rendered twice when recording and refused if the two runs differ. Needs a GPU.

    python scripts/plan_usage.py [--out tests/golden/plan_usage.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FIELDS = ("render_streams", "workspaces", "pass_samples", "workspace_bytes", "pair_passes", "split_passes",
          "deep_launch", "lead_tiles", "sky_tiles")
FRAMES = ((64, 36, 16), (64, 36, 96), (70, 37, 16), (70, 37, 96))
SEED, DEPTH = 1234, 64


def case_list():
    """The cases as plain records: scene, frame, options (rt.options fields), params flags
    (rt.make_params keywords), variance render or not, and the mode."""
    cases = []

    def add(name, W, H, spp, mode, scene="huge", options=None, flags=None, variance=False):
        opts = {"render_streams": 3}
        opts.update(options or {})
        if mode == "in_flight":
            opts["in_flight"] = 1
        cases.append({"name": f"{name} {W}x{H}x{spp} {mode}", "scene": scene, "width": W, "height": H, "spp": spp,
                      "mode": mode, "options": opts, "flags": flags or {}, "variance": variance})

    for W, H, spp in FRAMES:
        per_sample = W * H * 12
        dq = 256 << 10  # above the deep queue of one workspace at these frames (rt_plan.cpp deep_queue_bytes)
        shapes = [("defaults", {}), ("streams 1", {"render_streams": 1}), ("streams 7", {"render_streams": 7}),
                  ("one workspace per stream", {"workspaces_per_stream": 1}),
                  ("ring 32", {"ring_pass_bytes": 32 * per_sample}), ("ring 40", {"ring_pass_bytes": 40 * per_sample})]
        # from generous (every workspace whole) to one stream with 4-sample passes
        for n_ws, samples in ((8, spp), (3, spp), (2, 8), (1, 4)):
            cap = n_ws * (samples * per_sample + dq) + 2 * per_sample
            shapes.append((f"cap {n_ws} x {samples}", {"max_workspace_bytes": cap}))
        shapes += [("pairs", {"pairs": 1}), ("no deep split", {"deep_split": 0})]
        for mode in ("lone", "in_flight"):
            if mode == "in_flight" and (W, H, spp) not in ((64, 36, 96), (70, 37, 16)):
                continue
            for name, o in shapes:
                add(name, W, H, spp, mode, options=o)
            add("variance", W, H, spp, mode, variance=True)
            add("brute force", W, H, spp, mode, flags={"brute_force": True})
            add("wavefront", W, H, spp, mode, flags={"wavefront": True})
            add("simple scene", W, H, spp, mode, scene="simple")
    return cases


_scenes = {}


def run_case(case):
    """Renders the case on a fresh scene and returns the usage fields of FIELDS."""
    import torch

    import raytracinginoneweekend_amd as rt

    if case["scene"] not in _scenes:
        _scenes[case["scene"]] = rt.huge_scene_arrays(SEED) if case["scene"] == "huge" else rt.simple_scene_arrays()
    W, H, spp = case["width"], case["height"], case["spp"]
    cam = rt.Camera.default(W, H)
    p = rt.make_params(W, H, spp, DEPTH, SEED, **case["flags"])
    stream = torch.cuda.current_stream().cuda_stream
    ds = rt.DeviceScene(_scenes[case["scene"]], device=0, options=rt.options(**case["options"]))
    try:
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
        var = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
        for _ in range(2 if case["mode"] == "in_flight" else 1):
            if case["variance"]:
                ds.render_var(cam, p, out.data_ptr(), var.data_ptr(), stream)
            else:
                ds.render(cam, p, out.data_ptr(), stream)
        torch.cuda.synchronize()
        u = ds.usage()
    finally:
        ds.close()
    return {k: int(u[k]) for k in FIELDS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "plan_usage.json"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "plan_usage.py needs a GPU"
    torch.cuda.set_device(0)
    cases = case_list()
    for c in cases:
        c["usage"] = run_case(c)
        again = run_case(c)
        assert again == c["usage"], f"{c['name']}: two runs differ: {c['usage']} vs {again}"
        print(c["name"], c["usage"], flush=True)
    with open(args.out, "w") as f:
        json.dump({"fields": list(FIELDS), "cases": cases}, f, indent=1)
        f.write("\n")
    print(f"{len(cases)} cases -> {args.out}")


if __name__ == "__main__":
    main()
