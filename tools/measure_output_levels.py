"""tools/measure_output_levels.py — what the output levels and the gained PCM pack cost on the device (GPU box; bench.py does not
know them).

C2's batch (1024 contexts x 2 channels x 480 000 frames, bench.py's builder on a device-resident source) is built once and stays
resident; everything is timed in this one process.  The legs are run ALTERNATELY, ROUNDS rounds of STEPS timed calls each (after a
warm-up of every leg), and reported as the median of the rounds' medians with the round-to-round spread (min and max of those
medians):

    render              waa_render + waa_sync: the yardstick — the same code as the parent commit's, reading and writing 3.93 GB
    render_then_levels  the same followed by waa_output_levels
    levels              waa_output_levels alone (both kernels, 82 KB back), and per kernel from the library's profile slots
                        (device events around each launch) in rounds of their own
    level_series        waa_output_level_series alone (the same kernels, 92 MB back through the batch's staging block)
    pcm16 / pcm16_gain  waa_download_all_pcm16 against waa_download_all_pcm16_gain into the same pinned block; the pack kernels per
                        launch from the profile slots
    host_statistics     once per round: waa_download_all into a pinned block and the same five statistics in numpy on the host —
                        what a caller had to do before

The levels pass only READS the 3.93 GB the render reads and writes once each: if it takes longer than the render it is not bound
by memory, and the record says so (levels_over_render).

    python tools/measure_output_levels.py [--instances 1024] [--seconds 10] [--out profiles/output_levels_probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import web_audio_api_rs_amd as waa  # noqa: E402

SR = 48000.0
WARMUP, STEPS, ROUNDS = 3, 20, 5


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def summary(rounds):
    """rounds: a list of per-round medians (ms)"""
    return dict(ms=median(rounds), round_min_ms=min(rounds), round_max_ms=max(rounds), rounds_ms=rounds)


def wall(fn, steps=STEPS):
    """median wall ms of `steps` calls of fn (each ends in a device synchronise)"""
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return median(t)


def host_statistics(x):
    """the statistics of waa_level_stats with plain numpy on the downloaded planes [n, ch, frames] (any summation order)"""
    finite = np.isfinite(x)
    ax = np.abs(x)
    peak = np.where(finite, ax, 0).max(axis=2)
    sum_sq = np.einsum("ijk,ijk->ij", x, x, dtype=np.float64)
    v = x * np.float32(32768.0)
    clipped = ((v > 32767.0) | (v < -32768.0)).sum(axis=2)
    return peak, sum_sq, (~finite).sum(axis=2), clipped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "output_levels_probe.json"))
    args = ap.parse_args()
    n, frames = args.instances, int(args.seconds * SR) // 128 * 128
    hip = waa.default_binding()
    if hip.device_count() < 1:
        raise SystemExit("no HIP device: nothing here can be measured without one")
    noise = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    torch.cuda.synchronize()
    ctx, _ = bench.build_workload(waa, hip, "c2", n, frames, 0, noise.data_ptr())
    ctx.prepare()
    ctx.render_async()
    ctx.sync()
    h = ctx._handle
    pcm = torch.empty((n, frames, 2), dtype=torch.int16, pin_memory=True)
    pcm_p = C.cast(pcm.data_ptr(), C.POINTER(C.c_int16))
    gain = np.full(n, 0.5, np.float32)
    gain_p = waa.api._fp(gain)
    stats = np.zeros((n, 2), waa.api.LEVEL_STATS_DTYPE)
    stats_p = stats.ctypes.data_as(C.c_void_p)

    def render():
        ctx.render_async()
        ctx.sync()

    def levels():
        hip.check(hip.output_levels(h, stats_p))

    def render_then_levels():
        ctx.render_async()
        levels()

    legs = {
        "render": render, "render_then_levels": render_then_levels, "levels": levels, "level_series": ctx.output_level_series,
        "pcm16": lambda: hip.check(hip.download_all_pcm16(h, pcm_p)),
        "pcm16_gain": lambda: hip.check(hip.download_all_pcm16_gain(h, pcm_p, gain_p)),
    }
    for fn in legs.values():
        for _ in range(WARMUP):
            fn()
    rounds = {k: [] for k in legs}
    kernels = {}
    f32 = torch.empty((n, 2, frames), dtype=torch.float32, pin_memory=True)
    f32_np = f32.numpy()
    host = dict(download_ms=[], numpy_ms=[])
    for r in range(ROUNDS):
        for name, fn in legs.items():
            rounds[name].append(wall(fn, 5 if name.startswith("pcm16") or name == "level_series" else STEPS))
        # per kernel: the library's profile slots (events around every launch), in a pass of its own
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(STEPS):
            ctx.render_async()
            levels()
        for _ in range(3):
            legs["pcm16"]()
            legs["pcm16_gain"]()
        ctx.sync()
        for name, launches, ms in ctx.profile_entries():
            if launches:  # (per render / per call, whatever the number of launches in it)
                kernels.setdefault(name, []).append(ms / (3 if "pcm16" in name else STEPS))
        ctx.profile(False)
        if r >= 2:  # (seconds of host work per round: two rounds show its size)
            continue
        t0 = time.perf_counter()
        hip.check(hip.download_all(h, C.cast(f32.data_ptr(), C.POINTER(C.c_float))))
        t1 = time.perf_counter()
        host_stats = host_statistics(f32_np)
        t2 = time.perf_counter()
        host["download_ms"].append((t1 - t0) * 1e3)
        host["numpy_ms"].append((t2 - t1) * 1e3)
    # the device's values against the host's, loosely (another summation order): the tool measures, the tests compare bits
    levels()
    agree = bool(np.array_equal(stats["peak"], host_stats[0]) and np.allclose(stats["sum_sq"], host_stats[1], rtol=1e-9) and
                 np.array_equal(stats["n_nonfinite"], host_stats[2]) and np.array_equal(stats["n_clipped"], host_stats[3]))
    ctx.close()

    gb = n * 2 * frames * 4 / 1e9
    rec = dict(instances=n, channels=2, frames=frames, sample_rate=SR, warmup=WARMUP, steps=STEPS, rounds=ROUNDS, output_gb=gb,
               workspace_mb=n * 2 * ((frames + 127) // 128) * 12 / 1e6, device=torch.cuda.get_device_name(0),
               legs={k: summary(v) for k, v in rounds.items()}, kernels_ms={k: summary(v) for k, v in sorted(kernels.items())},
               host_statistics=dict(download_all=summary(host["download_ms"]), numpy=summary(host["numpy_ms"]), agrees_with_the_device=agree))
    lv, rd = rec["kernels_ms"]["output_levels_kernel"]["ms"], rec["legs"]["render"]["ms"]
    render_kernels = sum(v["ms"] for k, v in rec["kernels_ms"].items() if "levels" not in k and "level_rows" not in k and "pcm16" not in k)
    rec["derived"] = dict(levels_kernel_gb_per_s=gb / lv * 1e3, render_kernels_ms=render_kernels, render_gb_per_s=2 * gb / render_kernels * 1e3,
                          levels_over_render=lv / render_kernels, levels_call_over_render_wall=rec["legs"]["levels"]["ms"] / rd,
                          render_then_levels_minus_render_ms=rec["legs"]["render_then_levels"]["ms"] - rd,
                          pcm16_gain_minus_pcm16_ms=rec["legs"]["pcm16_gain"]["ms"] - rec["legs"]["pcm16"]["ms"],
                          host_path_ms=rec["host_statistics"]["download_all"]["ms"] + rec["host_statistics"]["numpy"]["ms"])
    for k, v in rec["legs"].items():
        print(f"{k:>20}: {v['ms']:9.3f} ms  [{v['round_min_ms']:.3f}, {v['round_max_ms']:.3f}]", flush=True)
    for k, v in rec["kernels_ms"].items():
        print(f"{k:>40}: {v['ms']:9.4f} ms  [{v['round_min_ms']:.4f}, {v['round_max_ms']:.4f}]", flush=True)
    print(json.dumps(rec["derived"], indent=1), json.dumps(rec["host_statistics"]["download_all"]["ms"]), json.dumps(rec["host_statistics"]["numpy"]["ms"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
