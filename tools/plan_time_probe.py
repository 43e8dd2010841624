"""tools/plan_time_probe.py [workload ...] — host planning time of bench.py's workloads on a PLAN-ONLY batch (no device: runs in
the authoring container): what build_plan costs on the host, per workload, best of 5.  The first render of a fresh batch pays
this once (bench.py's `one_shot` / first_render_ms).
A name of the form iirpi<order> is bench.py's iir<order> with one coefficient set per context (1024 distinct Butterworth sets): the
host cost of the scan kernel's matrix powers, computed once per distinct set.
dyn and qloop are no bench.py workloads: the graph of tools/dyn_probe.py (exact per-quantum channel counts: one dyn_kernel group)
and a feedback loop around an oversampled WaveShaper (dynamic counts, cut at the node and launched quantum block by block)."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bench  # noqa: E402
import web_audio_api_rs_amd as waa  # noqa: E402

hip = waa.default_binding()
names = sys.argv[1:] or ["c2", "t1", "c3", "c4", "c5", "c1a", "os2", "os4", "hrtf", "echo", "fb", "fbq", "fm", "osc", "trem", "dyn", "qloop"]
frames = 480000


def build_dynamic(name, n_inst):
    ctx = waa.OfflineAudioContext(2, frames, 48000.0, n_instances=n_inst, binding=hip, device=waa.PLAN_ONLY)
    mono, stereo = ctx.create_buffer_source(), ctx.create_buffer_source()
    mono.set_buffer(waa.AudioBuffer(np.zeros((1, frames), np.float32), 48000.0))
    stereo.set_buffer(waa.AudioBuffer(np.zeros((2, frames // 2), np.float32), 48000.0))
    mono.start()
    stereo.start_at(1.0)
    if name == "dyn":
        bq = ctx.create_biquad_filter(type_="lowpass", frequency=2000.0)
        mono.connect(bq)
        stereo.connect(bq)
        bq.connect(ctx.create_stereo_panner(pan=0.3)).connect(ctx.destination())
    else:
        d = ctx.create_delay(0.1, delay_time=0.01)
        sh = ctx.create_wave_shaper(curve=np.tanh(np.linspace(-2.5, 2.5, 129)).astype(np.float32), oversample="2x")
        mono.connect(d)
        stereo.connect(d)
        d.connect(sh).connect(ctx.create_gain(gain=0.45)).connect(d)
        sh.connect(ctx.destination())
    return ctx


for name in names:
    per_inst_order = int(name[5:]) if name.startswith("iirpi") else 0
    if per_inst_order:
        name = f"iir{per_inst_order}"
    n_inst = bench.DEFAULT_INSTANCES.get(name, 1024)
    best, head = 1e9, ""
    for rep in range(5):
        if name in ("dyn", "qloop"):
            ctx, src = build_dynamic(name, n_inst), None
        else:
            ctx, src = bench.build_workload(waa, hip, name, n_inst, frames, waa.PLAN_ONLY, None)
        if hasattr(src, "set_buffer") and name not in ("fm", "osc"):
            src.set_buffer(waa.AudioBuffer(np.zeros((2, 65536 if name == "c5" else frames), np.float32), 48000.0))
        if per_inst_order:
            from scipy import signal
            node = [nd for nd in ctx._nodes if isinstance(nd, waa.api.IIRFilterNode)][0]
            for i in range(n_inst):
                node.set_coefficients(*signal.butter(per_inst_order, 0.15 + 0.45 * i / (n_inst - 1)), instance=i)
        ctx.prepare()
        t0 = time.perf_counter()
        text = ctx.plan_describe()
        ms = (time.perf_counter() - t0) * 1e3
        if ms < best:
            best, head = ms, text.splitlines()[0].split("| timing: ")[-1]
        ctx.close()
    if per_inst_order:
        name += ",inst"
    print(f"{name:5s} {n_inst:5d} ctx  plan {best:8.2f} ms   {head}", flush=True)
