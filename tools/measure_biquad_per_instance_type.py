"""tools/measure_biquad_per_instance_type.py — what one filter type per context costs (DESIGN.md 3.1 "Per-context types").

1024 contexts x 10 s stereo at 48 kHz, the source resident on the device (adopted, as bench.py does).  Two workloads, each with ONE
type for the batch and with types i % 8:
  "c2"   BufferSource -> Biquad(constant params, a frequency per context) -> Gain(0.5) -> destination: the same kernel and the same
         bytes either way — the coefficient rows were per context already
  "c1a"  BufferSource -> Biquad(frequency: one exponential ramp 10 Hz -> 10 kHz scheduled on every context) -> destination: one type
         shares one per-frame table (40 B per frame), eight types need a row per context (40 B per frame and context)
Both legs of a workload live in the same process and are timed alternately: ROUNDS rounds of STEPS renders each, a host clock around
renders that end in a synchronise; the figure is the median over the rounds of the mean time per render, the spread the
(max - min) / median of the shared leg's rounds.  Needs a GPU; writes profiles/biquad_per_instance_type.json (or the path given as
the first argument)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import web_audio_api_rs_amd as waa  # noqa: E402

SR, N_INST, SECONDS = 48000.0, 1024, 10.0
WARMUP, STEPS, ROUNDS = 3, 20, 5
TYPES = tuple(waa.BIQUAD_TYPE)


def build(hip, noise, frames, workload, mixed):
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=N_INST, binding=hip, device=0)
    src = ctx.create_buffer_source()
    src.adopt_device_buffer(noise.data_ptr(), 2, frames, SR)
    bq = ctx.create_biquad_filter(type_="lowpass", frequency=200.0, q=1.0)
    if mixed:
        bq.set_type_batch([TYPES[i % 8] for i in range(N_INST)])
    if workload == "c2":
        for i in range(N_INST):
            bq.frequency.set_value(100.0 + 8.0 * i, instance=i)
        src.connect(bq).connect(ctx.create_gain(gain=0.5)).connect(ctx.destination())
    else:
        bq.frequency.set_value_at_time(10.0, 0.0)
        bq.frequency.exponential_ramp_to_value_at_time(10000.0, frames / SR)
        src.connect(bq).connect(ctx.destination())
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


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "biquad_per_instance_type.json")
    hip = waa.default_binding()
    if hip.device_count() < 1:
        raise RuntimeError("this measurement needs a GPU")
    frames = int(round(SECONDS * SR))
    frames_padded = (frames + 2047) // 2048 * 2048
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0xA0D10)
    noise = torch.empty((N_INST, 2, frames), dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0, generator=gen)
    torch.cuda.synchronize()
    record = {"contexts": N_INST, "seconds": SECONDS, "channels": 2, "sample_rate": SR, "warmup": WARMUP, "steps": STEPS, "rounds": ROUNDS,
              "device": torch.cuda.get_device_name(0), "signal_gb": round(N_INST * 2 * frames * 4 / 1e9, 3), "workloads": {}}
    for workload in ("c2", "c1a"):
        forms = {"shared": build(hip, noise, frames, workload, False), "mixed": build(hip, noise, frames, workload, True)}
        plans = {k: [l for l in c.plan_describe().splitlines() if l.startswith(("biquad", "chain"))] for k, c in forms.items()}
        for c in forms.values():
            window(c, WARMUP)
        ms = {k: [] for k in forms}
        for _ in range(ROUNDS):
            for k, c in forms.items():  # alternating
                ms[k].append(window(c, STEPS))
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = {"shared_ms": round(med["shared"], 4), "mixed_ms": round(med["mixed"], 4), "ratio": round(med["mixed"] / med["shared"], 4),
               "shared_spread": round((max(ms["shared"]) - min(ms["shared"])) / med["shared"], 4),
               "shared_ms_rounds": [round(v, 4) for v in ms["shared"]], "mixed_ms_rounds": [round(v, 4) for v in ms["mixed"]], "plans": plans}
        if workload == "c1a":  # the per-frame table: 5 f64 per frame of a padded row
            rows = {k: N_INST if any("per-instance table" in l for l in plans[k]) else 1 for k in forms}
            rec["table_bytes"] = {k: rows[k] * frames_padded * 40 for k in forms}
        record["workloads"][workload] = rec
        for c in forms.values():
            c.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps({w: {k: v for k, v in r.items() if k != "plans"} for w, r in record["workloads"].items()}))


if __name__ == "__main__":
    main()
