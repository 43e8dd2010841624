"""tools/measure_panner_per_instance_options.py — what one PannerNode option set per context costs.

1024 contexts x 10 s at 48 kHz, stereo BufferSource -> equal-power PannerNode -> destination, the source resident on the device
(adopted, as bench.py does).  Three cases, each with ONE option set for the batch and with the sets OPTIONS[i % 13] of
tests/test_panner_geometry.py:
  "a"  a constant position per context, the listener at rest: the geometry is evaluated on the host at plan time into gain tables
       that were per context already — the same kernels and the same bytes either way
  "b"  the listener's positionX audio-rate, a linear ramp of its own per context: seven per-frame tables with a row per context in
       both legs, written by panner_geom_kernel (one set) or panner_geom_inst_kernel (a set per context)
  "c"  ONE audio-rate listener ramp shared by the batch: one set shares one table row, differing sets need a row per context
       (7 tables x 4 B per frame and context)
Both legs of a case live in the same process and are timed alternately: ROUNDS rounds of STEPS renders each after WARMUP renders, a
host clock around renders that end in a synchronise; the figure is the median over the rounds of the mean time per render, the
spread the (max - min) / median of the shared leg's rounds.  Case "a" also records the host planning time of both legs on a
plan-only batch (the method of tools/plan_time_probe.py: best of 5).  Needs a GPU; writes profiles/panner_per_instance_options.json
(or the path given with --out).  `--only b --steps 3 --rounds 1 --out ...` is the short run a kernel trace is taken from."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import web_audio_api_rs_amd as waa  # noqa: E402
from test_panner_geometry import OPTIONS  # noqa: E402

SR, N_INST, SECONDS = 48000.0, 1024, 10.0
WARMUP, STEPS, ROUNDS = 3, 20, 5
SHARED_SET = OPTIONS[5]  # inverse, ref 1, rolloff 1, no cone: the constructor's defaults but for the outer gain


def position(i):
    return (1.0 + 0.01 * i, 0.5, -2.0 - 0.005 * i)


def build(hip, noise_ptr, frames, case, mixed, device=0):
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=N_INST, binding=hip, device=device)
    src = ctx.create_buffer_source()
    if noise_ptr is not None:
        src.adopt_device_buffer(noise_ptr, 2, frames, SR)
    else:  # (plan-only: the planner needs the buffer's shape alone)
        import numpy as np
        src.set_buffer(waa.AudioBuffer(np.zeros((2, frames), np.float32), SR))
    pn = ctx.create_panner(panning_model="equalpower", orientation=(0.3, -0.2, 1.0), position=position(0), **SHARED_SET)
    if mixed:
        pn.set_options_batch([OPTIONS[i % len(OPTIONS)] for i in range(N_INST)])
    lx = ctx.listener().position_x
    if case in ("a", "b"):
        for i in range(N_INST):
            for prm, v in zip(pn.params[:3], position(i)):
                prm.set_value(v, instance=i)
    if case == "b":
        for i in range(N_INST):
            lx.set_value_at_time(-4.0 + 0.002 * i, 0.0, instance=i)
            lx.linear_ramp_to_value_at_time(4.0 - 0.002 * i, frames / SR, instance=i)
    elif case == "c":
        lx.set_value_at_time(-4.0, 0.0)
        lx.linear_ramp_to_value_at_time(4.0, frames / SR)
    src.connect(pn).connect(ctx.destination())
    src.start()
    ctx.prepare()
    return ctx


def window(ctx, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.render_async()
    ctx.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def plan_time(hip, frames, mixed):
    """host planning of case "a" on a plan-only batch: (best wall ms of plan_describe over 5, the plan's own timing line)"""
    best, head = 1e9, ""
    for _ in range(5):
        ctx = build(hip, None, frames, "a", mixed, device=waa.PLAN_ONLY)
        t0 = time.perf_counter()
        text = ctx.plan_describe()
        ms = (time.perf_counter() - t0) * 1e3
        if ms < best:
            best, head = ms, text.splitlines()[0].split("| timing: ")[-1]
        ctx.close()
    return round(best, 3), head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panner_per_instance_options.json"))
    ap.add_argument("--only", default="abc")
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    hip = waa.default_binding()
    if hip.device_count() < 1:
        raise RuntimeError("this measurement needs a GPU")
    frames = int(round(SECONDS * SR))
    n_table_frames = (frames + 127) // 128 * 128
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0xA0D10)
    noise = torch.empty((N_INST, 2, frames), dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0, generator=gen)
    torch.cuda.synchronize()
    record = {"contexts": N_INST, "seconds": SECONDS, "channels": 2, "sample_rate": SR, "warmup": WARMUP, "steps": args.steps,
              "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "signal_gb": round(N_INST * 2 * frames * 4 / 1e9, 3),
              "option_sets": "tests/test_panner_geometry.py OPTIONS[i % 13]", "cases": {}}
    for case in args.only:
        forms = {"shared": build(hip, noise.data_ptr(), frames, case, False), "mixed": build(hip, noise.data_ptr(), frames, case, True)}
        plans = {k: [l for l in c.plan_describe().splitlines() if l.startswith(("panner", "chain"))] for k, c in forms.items()}
        kernels = {k: sorted(name for name, _, _ in c.profile_entries()) for k, c in forms.items()}
        for c in forms.values():
            window(c, WARMUP)
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, c in forms.items():  # alternating
                ms[k].append(window(c, args.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = {"shared_ms": round(med["shared"], 4), "mixed_ms": round(med["mixed"], 4), "ratio": round(med["mixed"] / med["shared"], 4),
               "shared_spread": round((max(ms["shared"]) - min(ms["shared"])) / med["shared"], 4),
               "shared_ms_rounds": [round(v, 4) for v in ms["shared"]], "mixed_ms_rounds": [round(v, 4) for v in ms["mixed"]], "plans": plans,
               "kernels": kernels}
        if case in ("b", "c"):  # seven f32 tables of n_quanta * 128 frames per row
            rows = {k: 1 if any("(1 table row(s))" in l for l in plans[k]) else N_INST for k in forms}
            rec["table_rows"] = rows
            rec["table_bytes"] = {k: rows[k] * n_table_frames * 7 * 4 for k in forms}
        if case == "a":
            rec["host_plan_ms"] = {}
            for k, mixed in (("shared", False), ("mixed", True)):
                best, head = plan_time(hip, frames, mixed)
                rec["host_plan_ms"][k] = {"plan_describe_best_of_5_ms": best, "timing": head}
        record["cases"][case] = rec
        for c in forms.values():
            c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps({w: {k: v for k, v in r.items() if k not in ("plans", "kernels")} for w, r in record["cases"].items()}))


if __name__ == "__main__":
    main()
