"""Times the display step (mpt_display to a device destination) at 1920x1080: the DEFAULT view
with tonemapping and the convergence heat map, the cost a front-end pays once per displayed
frame next to the batch-1 C3 frame.

Method: one adaptive sample of the Cornell box so that every buffer exists, then per view a
warm-up and `--launches` back-to-back launches on the context's stream between two stream
events (no host synchronisation inside the window).  Prints one JSON line per view: ms per
launch and the effective GB/s of the bytes the view must move (12 B read + 4 B written per
pixel; the heat map reads 4 B)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hiprt-path-tracer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch

    import mpt
    from mpt import abi, scene

    W, H = a.width, a.height
    stream = torch.cuda.Stream()
    sd = scene.load_scene("cornell_pbr")
    st = scene.parity_settings(3)
    st.enable_adaptive_sampling = True
    st.adaptive_sampling_min_samples = 1
    frame = scene.make_frame(scene.make_camera(sd.camera_info, W, H), W, H, settings=st)
    dst = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
        r.set_scene(sd)
        r.set_luts()
        r.render(frame)
        r.synchronize_kernel()
        for name, view, bytes_px in (("default_tonemapped", abi.VIEW_DEFAULT, 16), ("heat_map", abi.VIEW_PIXEL_CONVERGENCE_HEATMAP, 8)):
            s = r.display_settings(view)
            s.max_val = 4.0   # a gradient, not the min == max constant
            for _ in range(a.warmup):
                r.display_to_device(dst.data_ptr(), settings=s)
            r.synchronize_kernel()
            times = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.launches):
                    r.display_to_device(dst.data_ptr(), settings=s)
                e1.record(stream)
                e1.synchronize()
                times.append(e0.elapsed_time(e1) / a.launches)
            ms = sorted(times)[len(times) // 2]
            print(json.dumps({"view": name, "width": W, "height": H, "launches": a.launches, "ms_per_launch": round(ms, 5),
                              "ms_min": round(min(times), 5), "ms_max": round(max(times), 5),
                              "effective_GBps": round(W * H * bytes_px / (ms * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
