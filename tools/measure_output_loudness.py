"""tools/measure_output_loudness.py — what the integrated loudness costs on the device (GPU box; bench.py does not know it).

C2's batch (1024 contexts x 2 channels x 480 000 frames, bench.py's builder on a device-resident source) is built once and stays
resident; everything is timed in this one process.  The legs are run ALTERNATELY, ROUNDS rounds of STEPS timed calls each (after a
warm-up of every leg), and reported as the median of the rounds' medians with the round-to-round spread (min and max of those
medians):

    render                waa_render + waa_sync: the yardstick — reads and writes 3.93 GB once each
    levels                waa_output_levels: reads the same 3.93 GB once
    loudness              waa_output_loudness alone (three kernels, 1.6 MB of z back, gating on the host), and per kernel from the
                          library's profile slots (device events around each launch) in rounds of their own
    loudness_series       waa_output_loudness_series alone (the same kernels, z into caller memory, no gating)
    render_then_loudness  the render followed by the call
    pcm16                 waa_download_all_pcm16 into a pinned block: the download the call precedes.  A loudness call slower than
                          this has lost its point; the record says which kernel binds (derived.binding_kernel).

The loudness pass READS the 3.93 GB twice (zero-state pass, exact pass): derived.*_gb_per_s set each kernel against the levels
kernel's byte rate in the same process.

    python tools/measure_output_loudness.py [--instances 1024] [--seconds 10] [--out profiles/output_loudness_probe.json]"""
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
KERNELS = ("loudness_state_kernel", "loudness_chain_kernel", "loudness_energy_kernel")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "output_loudness_probe.json"))
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
    hop = int(hip.loudness_hop(SR))
    n_sub = frames // hop
    pcm = torch.empty((n, frames, 2), dtype=torch.int16, pin_memory=True)
    pcm_p = C.cast(pcm.data_ptr(), C.POINTER(C.c_int16))
    levels_out = np.zeros((n, 2), waa.api.LEVEL_STATS_DTYPE)
    levels_p = levels_out.ctypes.data_as(C.c_void_p)
    stats = np.zeros(n, waa.api.LOUDNESS_STATS_DTYPE)
    stats_p = stats.ctypes.data_as(C.c_void_p)
    z = np.zeros((n, 2, n_sub))
    z_p = z.ctypes.data_as(waa.api._DP)

    def render():
        ctx.render_async()
        ctx.sync()

    def levels():
        hip.check(hip.output_levels(h, levels_p))

    def loudness():
        hip.check(hip.output_loudness(h, None, stats_p))

    def render_then_loudness():
        ctx.render_async()
        loudness()

    legs = {
        "render": render, "levels": levels, "loudness": loudness,
        "loudness_series": lambda: hip.check(hip.output_loudness_series(h, z_p)),
        "render_then_loudness": render_then_loudness,
        "pcm16": lambda: hip.check(hip.download_all_pcm16(h, pcm_p)),
    }
    for fn in legs.values():
        for _ in range(WARMUP):
            fn()
    rounds = {k: [] for k in legs}
    kernels = {}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            rounds[name].append(wall(fn, 5 if name == "pcm16" else STEPS))
        # per kernel: the library's profile slots (events around every launch), in a pass of its own
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(STEPS):
            ctx.render_async()
            levels()
            loudness()
        ctx.sync()
        for name, launches, ms in ctx.profile_entries():
            if launches:  # (per render / per call, whatever the number of launches in it)
                kernels.setdefault(name, []).append(ms / STEPS)
        ctx.profile(False)
    loudness()
    ctx.close()

    gb = n * 2 * frames * 4 / 1e9
    rec = dict(instances=n, channels=2, frames=frames, sample_rate=SR, hop=hop, n_sub=n_sub, warmup=WARMUP, steps=STEPS, rounds=ROUNDS,
               output_gb=gb, workspace_mb=n * 2 * n_sub * 9 * 8 / 1e6, device=torch.cuda.get_device_name(0),
               legs={k: summary(v) for k, v in rounds.items()}, kernels_ms={k: summary(v) for k, v in sorted(kernels.items())},
               integrated_lufs=dict(min=float(stats["integrated"].min()), max=float(stats["integrated"].max())))
    k = {name: rec["kernels_ms"][name]["ms"] for name in KERNELS}
    lv = rec["kernels_ms"]["output_levels_kernel"]["ms"]
    call, pcm16 = rec["legs"]["loudness"]["ms"], rec["legs"]["pcm16"]["ms"]
    rec["derived"] = dict(levels_kernel_gb_per_s=gb / lv * 1e3, state_kernel_gb_per_s=gb * (n_sub - 1) / n_sub / k[KERNELS[0]] * 1e3,
                          energy_kernel_gb_per_s=gb / k[KERNELS[2]] * 1e3, kernels_sum_ms=sum(k.values()),
                          binding_kernel=max(k, key=k.get), loudness_over_levels_call=call / rec["legs"]["levels"]["ms"],
                          loudness_over_pcm16_download=call / pcm16, slower_than_the_pcm16_download=bool(call > pcm16),
                          render_then_loudness_minus_render_ms=rec["legs"]["render_then_loudness"]["ms"] - rec["legs"]["render"]["ms"])
    for name, v in rec["legs"].items():
        print(f"{name:>22}: {v['ms']:9.3f} ms  [{v['round_min_ms']:.3f}, {v['round_max_ms']:.3f}]", flush=True)
    for name, v in rec["kernels_ms"].items():
        print(f"{name:>40}: {v['ms']:9.4f} ms  [{v['round_min_ms']:.4f}, {v['round_max_ms']:.4f}]", flush=True)
    print(json.dumps(rec["derived"], indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
