"""tools/osc_types_probe.py — what one waveform type per context costs an OscillatorNode on the device (GPU box; bench.py does not
know the feature).

1024 contexts x 10 s at 48 kHz, one oscillator -> destination, a frequency per context (110 Hz ... 1.76 kHz), in ONE process:

 (a) each of the five types as a single-type batch (the kernels of waa_osc.hip; custom: 205 distinct 64-harmonic waves, one per
     context by i % 205, the all-custom per-instance-wave plan)
 (b) types i % 4 (sine / square / sawtooth / triangle)                       — the kernels of waa_osc_types.hip, 8 KB of LDS
 (c) types i % 5, the custom contexts with 205 distinct 64-harmonic waves    — the same, 32 KB of LDS per workgroup

for the time-parallel form (constant frequencies) and the prefix-sum form (the frequencies under one shared a-rate vibrato block;
the per-context part is then the detune).  Legs alternate REPS times over, each a fresh batch with a warm-up render, then ITERS
renders; the figure is the library's profile slot of the oscillator kernels (device events), per leg minimum, median, all
repetitions and their spread.  A mixed leg is judged against ITS MEMBER legs (a) of the same run (b: the four built-in types, c: all
five): between the fastest and the slowest of them, above the slowest by no more than that leg's spread.

 (d) the time-parallel mixed legs once more through the measurement build, the sine table staged in LDS (what the library runs)
     against read through the caches (WAA_OSC_TYPES_SINE_CACHED=1: the same bits), alternating like the legs above.

 --plan-time: no device — the host's planning time of the time-parallel legs on a plan-only batch (wall time of the first
 waa_plan_describe, three plans per leg), written to profiles/osc_types_plan_time.json.

    python tools/osc_types_probe.py [--plan-time] [--instances 1024] [--seconds 10] [--out profiles/osc_types_probe.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import web_audio_api_rs_amd as waa  # noqa: E402

SR = 48000.0
REPS, ITERS = 3, 3
TYPES = ("sine", "square", "sawtooth", "triangle", "custom")
N_WAVES, HARMONICS = 205, 64


def waves():
    rng = np.random.default_rng(0x05C7)
    j = np.arange(HARMONICS, dtype=np.float64)
    roll = np.where(j > 0, 1.0 / np.maximum(j, 1.0), 0.0)
    real, imag = (rng.uniform(-1.0, 1.0, (N_WAVES, HARMONICS)) * roll).astype(np.float32), (rng.uniform(-1.0, 1.0, (N_WAVES, HARMONICS)) * roll).astype(np.float32)
    return [waa.PeriodicWave(real=r, imag=i) for r, i in zip(real, imag)]


def graph(binding, n, frames, types, form, pw, device=0):
    ctx = waa.OfflineAudioContext(1, frames, SR, n_instances=n, binding=binding, device=device)
    osc = ctx.create_oscillator()
    if len(set(types)) == 1 and types[0] != "custom":
        osc.set_type(types[0])
    else:
        for i, t in enumerate(types):
            if t == "custom":
                osc.set_periodic_wave(pw[i % N_WAVES], instance=i)
            else:
                osc.set_type(t, instance=i)
    freq = 110.0 * 2.0 ** (4.0 * np.arange(n) / n)
    if form == "par":
        for i in range(n):
            osc.frequency.set_value(float(freq[i]), instance=i)
    else:
        k = np.arange(frames, dtype=np.float64)
        osc.frequency.set_block(0, (440.0 + 30.0 * np.sin(k * (2.0 * np.pi * 5.0 / SR))).astype(np.float32).reshape(-1, 128))
        for i in range(n):
            osc.detune.set_value(float(1200.0 * np.log2(freq[i] / 440.0)), instance=i)
    osc.connect(ctx.destination())
    osc.start()
    return ctx


def render_time(binding, n, frames, types, form, pw, switch=None):
    if switch:
        os.environ[switch] = "1"  # (read by the measurement build at every launch)
    try:
        return _render_time(binding, n, frames, types, form, pw)
    finally:
        if switch:
            os.environ.pop(switch, None)


def _render_time(binding, n, frames, types, form, pw):
    ctx = graph(binding, n, frames, types, form, pw)
    line = [l for l in ctx.plan_describe().splitlines() if l.startswith("oscillator node") and "frequency=" in l][0]
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


def plan_times(n, frames, out):
    import time
    hip, pw = waa.default_binding(), waves()
    legs = [("a: sine", ["sine"] * n), ("a: custom", ["custom"] * n), ("b: i % 4", [TYPES[i % 4] for i in range(n)]), ("c: i % 5", [TYPES[i % 5] for i in range(n)])]
    rec = dict(instances=n, frames=frames, what="wall ms of the first waa_plan_describe of a plan-only batch, time-parallel form, three plans per leg", legs={})
    for tag, types in legs:
        ms = []
        for _ in range(3):
            ctx = graph(hip, n, frames, types, "par", pw, device=waa.PLAN_ONLY)
            ctx.prepare()
            t0 = time.perf_counter()
            ctx.plan_describe()
            ms.append((time.perf_counter() - t0) * 1e3)
            ctx.close()
        rec["legs"][tag] = dict(ms_all=ms, ms_min=min(ms), ms_median=statistics.median(ms))
        print(tag, [round(v, 1) for v in ms], flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "osc_types_probe.json"))
    ap.add_argument("--plan-time", action="store_true")
    args = ap.parse_args()
    n, frames = args.instances, int(args.seconds * SR) // 2048 * 2048
    if args.plan_time:
        return plan_times(n, frames, os.path.join(os.path.dirname(os.path.abspath(args.out)), "osc_types_plan_time.json"))
    import torch
    hip, pw = waa.default_binding(), waves()
    legs = [(f"a: {t}", [t] * n) for t in TYPES] + [("b: i % 4", [TYPES[i % 4] for i in range(n)]), ("c: i % 5", [TYPES[i % 5] for i in range(n)])]
    rec = dict(instances=n, frames=frames, sample_rate=SR, reps=REPS, iters=ITERS, waves=N_WAVES, harmonics=HARMONICS,
               device=torch.cuda.get_device_name(0), forms={})
    for form in ("par", "scan"):
        runs, lines = {tag: [] for tag, _ in legs}, {}
        for rep in range(REPS):
            for tag, types in legs:
                lines[tag], k = render_time(hip, n, frames, types, form, pw)
                runs[tag].append(sum(k.values()))
                print(f"{form} rep {rep} {tag:12s} {sum(k.values()):8.3f} ms  {k}", flush=True)
        res = {tag: dict(plan=lines[tag], ms_min=min(v), ms_median=statistics.median(v), ms_all=v, spread_ms=max(v) - min(v)) for tag, v in runs.items()}
        single = {tag: r for tag, r in res.items() if tag.startswith("a:")}
        verdict = {}
        for tag in ("b: i % 4", "c: i % 5"):
            members = [t for t in single if tag.startswith("c") or "custom" not in t]
            slow = max(members, key=lambda t: single[t]["ms_median"])
            fast = min(members, key=lambda t: single[t]["ms_median"])
            verdict[tag] = dict(ms_median=res[tag]["ms_median"], mean_of_its_member_legs=statistics.mean(single[t]["ms_median"] for t in members),
                                fastest_member_leg=fast, slowest_member_leg=slow, over_the_slowest_member_ms=res[tag]["ms_median"] - single[slow]["ms_median"],
                                spread_of_the_slowest_member_ms=single[slow]["spread_ms"],
                                within=res[tag]["ms_median"] <= single[slow]["ms_median"] + single[slow]["spread_ms"])
        rec["forms"][form] = dict(legs=res, mixed=verdict)
        print(form, json.dumps(verdict), flush=True)
    # (d)
    measure = waa.measure_binding()
    variants = [(f"{tag}, sine table {how}", types, switch) for tag, types in legs[5:]
                for how, switch in (("staged in LDS", None), ("through the caches", "WAA_OSC_TYPES_SINE_CACHED"))]
    runs = {tag: [] for tag, *_ in variants}
    for rep in range(REPS):
        for tag, types, switch in variants:
            _, k = render_time(measure, n, frames, types, "par", pw, switch)
            runs[tag].append(sum(k.values()))
            print(f"(d) rep {rep} {tag:40s} {sum(k.values()):8.3f} ms", flush=True)
    rec["sine_table"] = {tag: dict(ms_min=min(v), ms_median=statistics.median(v), ms_all=v, spread_ms=max(v) - min(v)) for tag, v in runs.items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
