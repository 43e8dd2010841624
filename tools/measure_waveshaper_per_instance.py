"""tools/measure_waveshaper_per_instance.py — what one curve per context costs against the fused chain.

1024 contexts x 10 s stereo at 48 kHz, the source resident on the device (adopted, as bench.py does).  Two graphs, each rendered with
ONE shared 2048-point curve (the shaper fused into the chain kernel) and with 1024 distinct 2048-point curves (shaper_inst_kernel):
  "in place"   BufferSource -> WaveShaper -> destination         the per-instance kernel reads the source's AudioBuffer in place
  "behind a gain"  BufferSource -> Gain -> WaveShaper -> destination     the Gain's output is materialised in front of the per-instance node
Both forms live in the same process and are timed alternately: ROUNDS rounds of STEPS renders each, a host clock around renders that
end in a synchronise; the figure is the median over rounds of the mean time per render.  Needs a GPU; writes
profiles/waveshaper_per_instance.json (or the path given as the first argument)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import web_audio_api_rs_amd as waa  # noqa: E402

SR, N_INST, SECONDS, POINTS = 48000.0, 1024, 10.0, 2048
WARMUP, STEPS, ROUNDS = 3, 20, 5


def build(hip, noise, frames, graph, per_instance):
    ctx = waa.OfflineAudioContext(2, frames, SR, n_instances=N_INST, binding=hip, device=0)
    src = ctx.create_buffer_source()
    src.adopt_device_buffer(noise.data_ptr(), 2, frames, SR)
    x = np.linspace(-1.0, 1.0, POINTS)
    sh = ctx.create_wave_shaper(curve=None if per_instance else np.tanh(2.0 * x).astype(np.float32))
    if per_instance:
        sh.set_curve_batch([np.tanh((1.0 + 3.0 * i / N_INST) * x).astype(np.float32) for i in range(N_INST)])
    node = src.connect(ctx.create_gain(gain=0.8)) if graph == "behind a gain" else src
    node.connect(sh).connect(ctx.destination())
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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "waveshaper_per_instance.json")
    hip = waa.default_binding()
    if hip.device_count() < 1:
        raise RuntimeError("this measurement needs a GPU")
    frames = int(round(SECONDS * SR))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0xA0D10)
    noise = torch.empty((N_INST, 2, frames), dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0, generator=gen)
    torch.cuda.synchronize()
    signal_gb = N_INST * 2 * frames * 4 / 1e9
    tiles = (frames + 4095) // 4096
    record = {"contexts": N_INST, "seconds": SECONDS, "channels": 2, "sample_rate": SR, "curve_points": POINTS, "warmup": WARMUP, "steps": STEPS,
              "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "signal_gb": round(signal_gb, 3), "graphs": {}}
    for graph in ("in place", "behind a gain"):
        forms = {"shared": build(hip, noise, frames, graph, False), "per_instance": build(hip, noise, frames, graph, True)}
        plans = {k: [l for l in c.plan_describe().splitlines() if l.startswith(("chain", "shaper", "source node"))] for k, c in forms.items()}
        for c in forms.values():
            window(c, WARMUP)
        ms = {k: [] for k in forms}
        for _ in range(ROUNDS):
            for k, c in forms.items():  # alternating
                ms[k].append(window(c, STEPS))
        med = {k: statistics.median(v) for k, v in ms.items()}
        extra = 2 if graph == "behind a gain" else 0  # the Gain's output: written once, read once
        record["graphs"][graph] = {
            "shared_ms": round(med["shared"], 4), "per_instance_ms": round(med["per_instance"], 4),
            "ratio": round(med["per_instance"] / med["shared"], 4),
            "shared_ms_rounds": [round(v, 4) for v in ms["shared"]], "per_instance_ms_rounds": [round(v, 4) for v in ms["per_instance"]],
            # what each form has to move: the signals through HBM, and the curves (staged once per workgroup, from L2 after the first)
            "shared_gb": round(2 * signal_gb, 3), "per_instance_gb": round((2 + extra) * signal_gb, 3),
            "per_instance_curve_staging_gb": round(N_INST * tiles * POINTS * 4 / 1e9, 3), "distinct_curve_mb": round(N_INST * POINTS * 4 / 1e6, 3),
            "plans": plans}
        for c in forms.values():
            c.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps({g: {k: v for k, v in r.items() if k != "plans"} for g, r in record["graphs"].items()}))


if __name__ == "__main__":
    main()
