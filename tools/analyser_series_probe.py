"""tools/analyser_series_probe.py — what a whole series of AnalyserNode pulls costs on the device (GPU box; bench.py does not
know the feature).

1024 contexts x 10 s at 48 kHz of C2's graph (device-resident source -> Biquad -> Gain -> destination) with a series analyser AND
a plain analyser behind the gain: fft_size 2048 with a hop of 4 quanta, once unsmoothed (tau = 0) and once with tau = 0.8, then
fft_size 256 with a hop of 1.  Per kind of series (float / byte frequency data, float / byte time-domain data): the kernel time
from the library's profile slots, the bytes the kernels write and the fraction of the 8 TB/s peak those bytes make.

Yardstick, same process and same batch: the way to the same rows without the feature is one analyser_kernel launch per pull — the
profiled time of ONE pull of the plain analyser times the number of pulls P.  The series must come in below that product.  C2
itself (bench.py's builder) is timed in the same process as the box's yardstick.

Only instance 0's rows are copied to the host (the per-instance getter): the series of every instance is computed either way.

    python tools/analyser_series_probe.py [--instances 1024] [--seconds 10] [--out profiles/analyser_series_probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import web_audio_api_rs_amd as waa  # noqa: E402

SR = 48000.0
PEAK_BYTES_PER_S = 8e12
REPS = 3
KINDS = ("float_frequency", "byte_frequency", "float_time_domain", "byte_time_domain")


def graph(hip, noise, n, frames, fft, hop, tau):
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=n, binding=hip, device=0)
    src = ctx.create_buffer_source()
    src.adopt_device_buffer(noise.data_ptr(), 2, frames, SR)
    g = src.connect(ctx.create_biquad_filter(type_="lowpass", frequency=200.0, q=1.0)).connect(ctx.create_gain(gain=0.5))
    ser = ctx.create_analyser(fft_size=fft, smoothing_time_constant=tau, series_hop=hop, series_first=hop)
    plain = ctx.create_analyser(fft_size=fft, smoothing_time_constant=tau)
    g.connect(ser)
    g.connect(plain)
    g.connect(ctx.destination())
    src.start()
    return ctx, ser, plain


def pull_one(ctx, an, kind, rows, n):
    """the per-instance C getter for instance 0: [rows][n]"""
    dtype = np.float32 if "float" in kind else np.uint8
    out = np.zeros((rows, n), dtype)
    ptr = out.ctypes.data_as(waa.api._FP if dtype == np.float32 else C.POINTER(C.c_uint8))
    ctx._b.check(getattr(ctx._b, f"analyser_get_{kind}_data")(ctx._handle, an.id, 0, ptr, n))
    return out


def kernels(ctx):
    ctx.sync()
    return {name: ms for name, launches, ms in ctx.profile_entries() if launches}


def run(hip, noise, n, frames, fft, hop, tau):
    ctx, ser, plain = graph(hip, noise, n, frames, fft, hop, tau)
    P, M = len(ser.series_quanta), fft // 2
    ctx.prepare()
    ctx.render_async()
    ctx.sync()
    ctx.profile(True)
    best, single, renders = {}, [], []
    bins, samples = n * P * M, n * P * fft
    for rep in range(REPS + 1):  # (the first repetition allocates the series buffers: not recorded; from then on every kind has one)
        ctx.profile_reset()
        ctx.render_async()
        render_ms = sum(kernels(ctx).values())
        # Every kind has a buffer, so ONE pass serves a family whichever kind is asked for first: the first frequency pull runs
        # the transform stage (and the recursion) and writes float and byte rows, the first time-domain pull gathers both forms;
        # the second pull of a family launches nothing.  Bytes first on odd repetitions.
        bytes_first = rep % 2 == 1
        order = ("byte_frequency", "float_frequency", "byte_time_domain", "float_time_domain") if bytes_first else KINDS
        for kind in order:
            ctx.profile_reset()
            pull_one(ctx, ser, kind, P, fft if "time" in kind else M)
            k = {name: ms for name, ms in kernels(ctx).items() if name.startswith("analyser_series")}
            if not k or not rep:
                continue
            if "time" in kind:
                key, wrote = "time_domain float + byte rows, one gather", 5 * samples
            else:  # (tau > 0: the transform stage writes the magnitudes, the recursion rewrites them as dB and writes the bytes)
                key, wrote = "frequency float + byte rows, one pass", (5 if tau == 0 else 4 + 5) * bins
            if key not in best or sum(k.values()) < best[key]["ms"]:
                best[key] = dict(kernels_ms=k, ms=sum(k.values()), bytes_written=wrote)
        ctx.profile_reset()
        pull_one(ctx, plain, "float_frequency", 1, M)
        if rep:
            single.append(kernels(ctx)["analyser_kernel"])
            renders.append(render_ms)
    ctx.profile(False)
    ctx.close()
    one_pull_ms = min(single)
    line = dict(fft_size=fft, hop=hop, smoothing=tau, pulls=P, render_kernels_ms=min(renders), single_pull_ms=one_pull_ms,
                pull_per_launch_ms=one_pull_ms * P, kinds=best)
    for v in best.values():
        v["fraction_of_peak"] = v["bytes_written"] / (v["ms"] * 1e-3) / PEAK_BYTES_PER_S
    full = line["kinds"]["frequency float + byte rows, one pass"]
    freq_ms = full["ms"]
    line["series_over_per_launch"] = freq_ms / line["pull_per_launch_ms"]
    print(f"fft {fft} H {hop} tau {tau}: P = {P}; frequency series (float + byte rows) {freq_ms:.3f} ms "
          f"({full['fraction_of_peak']:.3f} of 8 TB/s) against {P} x {one_pull_ms:.4f} = {line['pull_per_launch_ms']:.2f} ms "
          f"of single pulls: ratio {line['series_over_per_launch']:.4f}; render {line['render_kernels_ms']:.3f} ms", flush=True)
    for key, v in line["kinds"].items():
        print(f"    {key:44s} {v['ms']:9.3f} ms  {v['bytes_written'] / 1e9:7.3f} GB  {v['fraction_of_peak']:.3f} of peak  {v['kernels_ms']}", flush=True)
    assert freq_ms < line["pull_per_launch_ms"], "the series must cost less than one launch per pull"
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analyser_series_probe.json"))
    args = ap.parse_args()
    n, frames = args.instances, int(args.seconds * SR) // 128 * 128
    hip = waa.default_binding()
    noise = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    torch.cuda.synchronize()
    rec = dict(instances=n, frames=frames, sample_rate=SR, reps=REPS, device=torch.cuda.get_device_name(0), peak_bytes_per_s=PEAK_BYTES_PER_S,
               lines=[])
    c2, _ = bench.build_workload(waa, hip, "c2", n, frames, 0, noise.data_ptr())
    c2.prepare()
    c2.render_async()
    c2.sync()
    c2.profile(True)
    c2_ms = []
    for _ in range(5):
        c2.profile_reset()
        c2.render_async()
        c2_ms.append(sum(kernels(c2).values()))
    c2.close()
    rec["c2_kernels_ms"] = min(c2_ms)
    print(f"C2 (same process): kernels {rec['c2_kernels_ms']:.3f} ms", flush=True)
    for fft, hop, tau in ((2048, 4, 0.0), (2048, 4, 0.8), (256, 1, 0.0)):
        rec["lines"].append(run(hip, noise, n, frames, fft, hop, tau))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
