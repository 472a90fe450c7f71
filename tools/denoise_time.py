"""Times the denoiser (mpt_denoise with a device-resident result, GPURenderer.denoise_to_device) at
1920x1080 on a 4-sample Cornell render with the default settings.

Method: per variant a warm-up, then `--calls` back-to-back calls on the context's stream between
two stream events (no host synchronisation inside the window), `--repeats` times with the
variants alternating inside every repeat; the median over the repeats is reported, with the
minimum and the maximum.  Variants (MPT_DENOISE_TILED, a bit mask over log2 step, read by the
library at every call): the table the library ships, the plain gather at every step, the tiled
kernel at every step, and the tiled kernel at one step only (the gather at the others).  One
mpt_display of the default view is timed the same way for scale.  Prints one JSON line.

--variant NAME runs only that variant, `--calls` times, with no events: the run to put under
`rocprofv3 --kernel-trace --stats` for per-kernel times."""
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
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=0, help="0: the default settings' (5)")
    ap.add_argument("--variant", default=None)
    a = ap.parse_args()
    import torch

    import mpt
    from mpt import abi, scene

    W, H = a.width, a.height
    stream = torch.cuda.Stream()
    sd = scene.load_scene("cornell_pbr")
    cam = scene.make_camera(sd.camera_info, W, H)
    frames = []
    for k, seed in scene.cpu_seed_schedule(4):
        st = scene.parity_settings(3)
        st.denoiser_AOV_accumulation_counter = k
        frames.append(scene.make_frame(cam, W, H, settings=st, sample_number=k, random_seed=seed))
    iters = a.iterations or abi.DenoiseSettings.default().iterations
    variants = {"table": None, "gather": 0, "tiled": (1 << iters) - 1}
    variants.update({f"tiled_step{1 << i}": 1 << i for i in range(iters)})

    def select(name):
        if variants[name] is None:
            os.environ.pop("MPT_DENOISE_TILED", None)
        else:
            os.environ["MPT_DENOISE_TILED"] = str(variants[name])

    dst = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    with mpt.GPURenderer(0, stream=stream.cuda_stream) as r:
        r.set_scene(sd)
        r.set_luts()
        r.render_samples(frames)
        r.synchronize_kernel()
        s = r.denoise_settings()
        s.iterations = iters
        if a.variant:
            select(a.variant)
            for _ in range(a.calls):
                r.denoise_to_device(None, s)
            r.synchronize_kernel()
            return

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.calls):
                fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / a.calls

        ds = r.display_settings(abi.VIEW_DEFAULT)
        runs = {name: (lambda: r.denoise_to_device(None, s)) for name in variants}
        runs["display_default"] = lambda: r.display_to_device(dst.data_ptr(), settings=ds)
        for name, fn in runs.items():
            select(name if name in variants else "table")
            for _ in range(a.warmup):
                fn()
        r.synchronize_kernel()
        times = {name: [] for name in runs}
        for _ in range(a.repeats):
            for name, fn in runs.items():
                select(name if name in variants else "table")
                times[name].append(timed(fn))
        select("table")
        out = {"width": W, "height": H, "samples": 4, "iterations": iters, "calls": a.calls, "repeats": a.repeats}
        for name, t in times.items():
            t = sorted(t)
            out[name] = {"ms": round(t[len(t) // 2], 4), "min": round(t[0], 4), "max": round(t[-1], 4)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
