"""tools/periodic_wave_probe.py — what one PeriodicWave per context costs an OscillatorNode on the device (GPU box; bench.py does
not know the feature).

1024 contexts x 10 s at 48 kHz, one custom oscillator with a constant frequency (the time-parallel kernel) -> destination, 64
harmonics per wave, the same 220 Hz everywhere (one replay row: what differs between the variants is the table alone), in ONE process:

 (a) plan time   1024 distinct coefficient sets, their tables generated on the device: wall time of the plan up to an idle stream,
                 beside the time 1024 calls of the host generator (waa_oscillator_set_periodic_wave) take in the same process — what
                 a caller paid per batch of 1024 timbres before, one batch per wave
 (b) generator   periodic_wave_kernel's own time for those 1024 tables, launch to idle: a child process with the measurement
                 build and WAA_PLAN_TRACE=1 (--generator-child), its "[plan]" line read from stderr
 (c) render      1024 distinct tables against ONE shared table (the same graph in shared mode), alternating REPS times over after a
                 warm-up render each, ITERS renders per repetition, the library's profile slot of the oscillator kernel; per variant
                 minimum, median and all repetitions, so that the spread of repeats stands beside the difference.  The
                 per-instance variant twice more through the measurement build: its table staged in LDS (osc_par_lds_kernel, what
                 the library runs) and read from global memory (WAA_OSC_NO_LDS_TABLE=1: osc_par_kernel with the row lookup).
                 --parent-lib: the shared variant through another build of the library as well (the parent commit's).

    python tools/periodic_wave_probe.py [--instances 1024] [--seconds 10] [--harmonics 64] [--parent-lib path/libwaa_hip.so]
                                        [--out profiles/periodic_wave_probe.json]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import web_audio_api_rs_amd as waa  # noqa: E402

SR = 48000.0
REPS, ITERS = 5, 5


def coefficient_sets(n, harmonics):
    """n distinct additive timbres: 1 / j roll-off with random weights and phases"""
    rng = np.random.default_rng(0x7ABE)
    j = np.arange(harmonics, dtype=np.float64)
    roll = np.where(j > 0, 1.0 / np.maximum(j, 1.0), 0.0)
    return (rng.uniform(-1.0, 1.0, (n, harmonics)) * roll).astype(np.float32), (rng.uniform(-1.0, 1.0, (n, harmonics)) * roll).astype(np.float32)


def graph(binding, n, frames, real, imag, per_instance, device=0):
    ctx = waa.OfflineAudioContext(1, frames, SR, n_instances=n, binding=binding, device=device)
    if per_instance:
        osc = ctx.create_oscillator(frequency=220.0)
        osc.set_periodic_wave_batch(real, imag)
    else:
        osc = ctx.create_oscillator(frequency=220.0, periodic_wave=waa.PeriodicWave(real=real[0], imag=imag[0]))
    osc.connect(ctx.destination())
    osc.start()
    return ctx


def plan_time(binding, n, frames, real, imag):
    ctx = graph(binding, n, frames, real, imag, True)
    ctx.prepare()
    ctx.sync()
    t0 = time.perf_counter()
    text = ctx.plan_describe()
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3
    note = [l for l in text.splitlines() if "one PeriodicWave per instance" in l][0]
    ctx.close()
    return ms, note, text.splitlines()[0].split(" | ")[1]


def host_generator_time(binding, real, imag):
    """the host generator, once per set, on a plan-only batch of one context (nothing else in the loop but the call)"""
    ctx = waa.OfflineAudioContext(1, 128, SR, binding=binding, device=waa.PLAN_ONLY)
    osc = ctx.create_oscillator()
    osc.connect(ctx.destination())
    ctx.prepare()
    fp = ctypes.POINTER(ctypes.c_float)
    t0 = time.perf_counter()
    for r, i in zip(real, imag):
        binding.check(binding.oscillator_set_periodic_wave(ctx._handle, osc.id, r.ctypes.data_as(fp), i.ctypes.data_as(fp), r.size, 0))
    ms = (time.perf_counter() - t0) * 1e3
    ctx.close()
    return ms


def render_time(binding, n, frames, real, imag, per_instance, switch=None):
    if switch:
        os.environ[switch] = "1"  # (read by the measurement build at every launch)
    try:
        ctx = graph(binding, n, frames, real, imag, per_instance)
        line = [l for l in ctx.plan_describe().splitlines() if l.startswith("oscillator node") and "custom (" in l][0]
        ctx.render_async()
        ctx.sync()
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(ITERS):
            ctx.render_async()
        ctx.sync()
        kernels = {name: ms / ITERS for name, launches, ms in ctx.profile_entries() if launches}
        ctx.close()
    finally:
        if switch:
            os.environ.pop(switch, None)
    return line, kernels


def generator_child(n, harmonics):
    """(b), in the child: plan a small render of n distinct sets; the library prints the kernel's time on stderr"""
    real, imag = coefficient_sets(n, harmonics)
    for k in (2, n):  # (two sets first: the first launch of a process loads the code object; the parent reads the LAST line)
        ctx = graph(waa.default_binding(), k, 2048, real[:k], imag[:k], True)
        ctx.plan_describe()
        ctx.sync()
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--harmonics", type=int, default=64)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--generator-child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic_wave_probe.json"))
    args = ap.parse_args()
    n, frames = args.instances, int(args.seconds * SR) // 2048 * 2048
    if args.generator_child:
        return generator_child(n, args.harmonics)
    import torch
    hip = waa.default_binding()
    real, imag = coefficient_sets(n, args.harmonics)
    rec = dict(instances=n, frames=frames, harmonics=args.harmonics, sample_rate=SR, reps=REPS, iters=ITERS, device=torch.cuda.get_device_name(0))
    # (a)
    warm = graph(hip, 2, 2048, real[:2], imag[:2], True)  # (the first plan of a process loads the code object)
    warm.plan_describe()
    warm.sync()
    warm.close()
    plans = [plan_time(hip, n, frames, real, imag) for _ in range(3)]
    host_ms = host_generator_time(hip, real, imag)
    rec["plan"] = dict(device_generated_plan_ms=[p[0] for p in plans], device_generated_plan_ms_min=min(p[0] for p in plans), note=plans[0][1],
                       timing_line=plans[-1][2], host_generator_ms_for_all_sets=host_ms, host_generator_ms_per_set=host_ms / n)
    print(f"(a) plan with {n} sets generated on the device: {[round(p[0], 2) for p in plans]} ms  [{plans[0][1]}]", flush=True)
    print(f"(a) {n} calls of the host generator: {host_ms:.1f} ms ({host_ms / n:.2f} ms per set)", flush=True)
    # (b)
    env = dict(os.environ, WAA_USE_MEASURE_LIB="1", WAA_PLAN_TRACE="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--generator-child", "--instances", str(n), "--harmonics", str(args.harmonics)],
                           env=env, stderr=subprocess.PIPE, text=True, timeout=300)
    m = re.findall(r"periodic_wave_kernel \(launch to idle\)\s+([0-9.]+) ms", child.stderr)
    if child.returncode != 0 or len(m) != 2:
        sys.stderr.write(child.stderr)
        raise SystemExit("the generator child did not report the kernel's time")
    rec["generator_kernel_ms"] = float(m[-1])
    print(f"(b) periodic_wave_kernel, {n} tables of {args.harmonics} harmonics: {rec['generator_kernel_ms']:.3f} ms", flush=True)
    # (c)
    measure = waa.measure_binding()
    variants = [("shared", hip, False, None), ("per-instance", hip, True, None),
                ("per-instance, table in LDS (measurement build)", measure, True, None),
                ("per-instance, table from global memory (measurement build)", measure, True, "WAA_OSC_NO_LDS_TABLE")]
    if args.parent_lib:
        variants.append(("shared (parent)", waa.bind(ctypes.CDLL(os.path.abspath(args.parent_lib)), "waa_"), False, None))
    runs, lines = {tag: [] for tag, *_ in variants}, {}
    for rep in range(REPS):
        for tag, binding, per_instance, switch in variants:
            lines[tag], k = render_time(binding, n, frames, real, imag, per_instance, switch)
            runs[tag].append(sum(k.values()))
            print(f"(c) rep {rep} {tag:60s} {sum(k.values()):8.3f} ms  {k}", flush=True)
    rec["render"] = {tag: dict(plan=lines[tag], ms_min=min(v), ms_median=statistics.median(v), ms_all=v, spread_ms=max(v) - min(v),
                               bytes_per_s_at_min=4.0 * n * frames / (min(v) * 1e-3)) for tag, v in runs.items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
