"""tools/iir_instance_probe.py — what one coefficient set per context costs an IIRFilterNode on the device (GPU box; bench.py does
not know the feature).

1024 contexts x 10 s x 2 channels at 48 kHz, device-resident source -> IIRFilter(Butterworth, order 4 and order 8) -> destination,
in ONE process and on ONE source allocation, the variants alternating REPS times over so that drift shows:

    shared            one set for the batch (waa_iir_set_coefficients): today's path, the scan kernel's shared form
    per-instance      1024 distinct sets (cut-offs spread over [0.15, 0.6]): the scan kernel's per-instance form, which reads its
                      coefficients and up to 6 ns^2 matrix entries per wave and tile from its instance's block
    per-instance row  the same sets through the exact row kernel (WAA_IIR_EXACT=1): what the planner would pick instead if the
                      per-instance scan were the slower one
    shared (parent)   --parent-lib: the shared variant through another build of the library (the parent commit's), tools/ab_lib.py's way

Times are the library's profile slots (HIP events around each kernel), ITERS renders per repetition behind one warm-up render;
per variant the minimum and the median over the repetitions are recorded, with the plan line that says which kernel ran.

    python tools/iir_instance_probe.py [--instances 1024] [--seconds 10] [--parent-lib path/libwaa_hip.so] [--out profiles/iir_per_instance.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import signal  # noqa: E402

import web_audio_api_rs_amd as waa  # noqa: E402

SR = 48000.0
REPS, ITERS = 3, 5


def graph(binding, noise, n, frames, order, per_instance):
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=n, binding=binding, device=0)
    src = ctx.create_buffer_source()
    src.adopt_device_buffer(noise.data_ptr(), 2, frames, SR)
    iir = ctx.create_iir_filter(*signal.butter(order, 0.3))
    if per_instance:
        for i in range(n):
            iir.set_coefficients(*signal.butter(order, 0.15 + 0.45 * i / max(1, n - 1)), instance=i)
    src.connect(iir).connect(ctx.destination())
    src.start()
    return ctx


def measure(binding, noise, n, frames, order, per_instance, exact):
    if exact:
        os.environ["WAA_IIR_EXACT"] = "1"
    try:
        ctx = graph(binding, noise, n, frames, order, per_instance)
        line = [l for l in ctx.plan_describe().splitlines() if l.startswith("iir_")][0].split(" | ")[0]
    finally:
        os.environ.pop("WAA_IIR_EXACT", None)
    ctx.render_async()
    ctx.sync()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(ITERS):
        ctx.render_async()
    ctx.sync()
    kernels = {name: ms / ITERS for name, launches, ms in ctx.profile_entries() if launches}
    ctx.close()
    return line, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iir_per_instance.json"))
    args = ap.parse_args()
    n, frames = args.instances, int(args.seconds * SR) // 2048 * 2048
    hip = waa.default_binding()
    variants = [("shared", hip, False, False), ("per-instance", hip, True, False), ("per-instance row", hip, True, True)]
    if args.parent_lib:
        variants.append(("shared (parent)", waa.bind(ctypes.CDLL(os.path.abspath(args.parent_lib)), "waa_"), False, False))
    noise = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    torch.cuda.synchronize()
    rec = dict(instances=n, frames=frames, channels=2, sample_rate=SR, reps=REPS, iters=ITERS, device=torch.cuda.get_device_name(0), orders={})
    for order in (4, 8):
        runs = {tag: [] for tag, *_ in variants}
        lines = {}
        for rep in range(REPS):
            for tag, binding, per_instance, exact in variants:
                lines[tag], k = measure(binding, noise, n, frames, order, per_instance, exact)
                runs[tag].append(sum(k.values()))
                print(f"order {order} rep {rep} {tag:18s} {sum(k.values()):8.3f} ms  {k}  [{lines[tag]}]", flush=True)
        bytes_moved = 2.0 * n * 2 * frames * 4  # one read and one write of every sample
        rec["orders"][str(order)] = {tag: dict(plan=lines[tag], ms_min=min(v), ms_median=statistics.median(v), ms_all=v,
                                               bytes_per_s_at_min=bytes_moved / (min(v) * 1e-3)) for tag, v in runs.items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
