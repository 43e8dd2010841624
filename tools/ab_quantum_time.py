#!/usr/bin/env python
"""tools/ab_quantum_time.py <other.so> — kernel times of the quantum-serial kernels (dyn_kernel, loop_kernel) through this tree's
measurement build and through another one (e.g. the parent commit's), both in one process, alternating AB_REPS (3) times, AB_ITERS
(3) renders each, HIP-event times from profile_entries().  1024 contexts x 10 s:
  * tools/dyn_probe.py's graph (a mono source plus a stereo one that starts late into Biquad -> StereoPanner), as planned and with
    WAA_DYN_NO_PIPE=1 (dyn_kernel<2, 1>);
  * the same graph with WAA_DYN_STAGES=2, and the same sources into Delay -> Biquad and into Biquad -> StereoPanner -> Gain
    (other stage counts: the instantiations dyn_kernel<2, W> differ in registers); the plan's stage count is printed with each;
  * bench.py's filtered feedback echo (fbq) with WAA_LOOP_KERNEL=1 (loop_kernel).
Per graph: every repeat, then the other build's and this tree's mean, min and max — the other build's own spread is the bar.  (GPU box)"""
import ctypes
import os
os.environ.setdefault("WAA_USE_MEASURE_LIB", "1")  # A/B and probe tools flip measurement switches: libwaa_hip_measure.so
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import web_audio_api_rs_amd as waa  # noqa: E402

SR = 48000.0
REPS = int(os.environ.get("AB_REPS", "3"))
ITERS = int(os.environ.get("AB_ITERS", "3"))
N_INST, FRAMES = 1024, 480000
_sources = {}


def dyn_graph(be, nodes):
    """b = Biquad, p = StereoPanner, g = Gain, d = Delay, in a row behind the two sources of tools/dyn_probe.py"""
    if not _sources:
        rng = np.random.default_rng(0)
        _sources["a"] = rng.uniform(-1, 1, (N_INST, 1, FRAMES)).astype(np.float32)
        _sources["b"] = rng.uniform(-1, 1, (N_INST, 2, FRAMES // 2)).astype(np.float32)
    ctx = waa.OfflineAudioContext(2, FRAMES, SR, n_instances=N_INST, binding=be)
    a = ctx.create_buffer_source()
    a.set_buffer_batch(_sources["a"], SR)
    b = ctx.create_buffer_source()
    b.set_buffer_batch(_sources["b"], SR)
    make = {"b": lambda: ctx.create_biquad_filter(type_="lowpass", frequency=2000.0), "p": lambda: ctx.create_stereo_panner(pan=0.3),
            "g": lambda: ctx.create_gain(gain=0.7), "d": lambda: ctx.create_delay(0.1, delay_time=0.01)}
    chain = [make[k]() for k in nodes]
    a.connect(chain[0])
    b.connect(chain[0])
    for x, y in zip(chain, chain[1:]):
        x.connect(y)
    chain[-1].connect(ctx.destination())
    a.start()
    b.start_at(1.0)
    return ctx


def timed(ctx, want):
    ctx.prepare()
    ctx.render_async()
    ctx.sync()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(ITERS):
        ctx.render_async()
    ctx.sync()
    r = {n: ms / ITERS for n, launches, ms in ctx.profile_entries() if launches and want in n}
    ctx.close()
    return r


def main(argv):
    other = os.path.basename(argv[0])
    libs = [(other, waa.bind(ctypes.CDLL(os.path.abspath(argv[0])), "waa_")), ("this tree", waa.measure_binding())]
    noise = torch.empty((N_INST, 2, FRAMES), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    fbq = lambda be: bench.build_workload(waa, be, "fbq", N_INST, FRAMES, 0, noise.data_ptr())[0]  # noqa: E731
    cases = [("dyn_probe, as planned", {}, lambda be: dyn_graph(be, "bp"), "dyn_kernel", "pipelined over the quanta"),
             ("dyn_probe, WAA_DYN_NO_PIPE=1", {"WAA_DYN_NO_PIPE": "1"}, lambda be: dyn_graph(be, "bp"), "dyn_kernel", "dynamic-count group"),
             ("dyn_probe, WAA_DYN_STAGES=2", {"WAA_DYN_STAGES": "2"}, lambda be: dyn_graph(be, "bp"), "dyn_kernel", "pipelined over the quanta"),
             ("Delay -> Biquad", {}, lambda be: dyn_graph(be, "db"), "dyn_kernel", "pipelined over the quanta"),
             ("Biquad -> StereoPanner -> Gain", {}, lambda be: dyn_graph(be, "bpg"), "dyn_kernel", "pipelined over the quanta"),
             ("fbq, WAA_LOOP_KERNEL=1", {"WAA_LOOP_KERNEL": "1"}, fbq, "loop_kernel", "feedback loop: ")]
    for name, env, build, want, plan_says in cases:
        os.environ.update(env)
        res = {tag: [] for tag, _ in libs}
        stages = "-"
        for rep in range(REPS):
            for tag, be in libs:
                ctx = build(be)
                plan = ctx.plan_describe()
                assert plan_says in plan, (name, plan_says, plan)
                if "pipelined over the quanta in " in plan and "WAA_DYN_NO_PIPE" not in env:
                    stages = plan.split("pipelined over the quanta in ")[1].split()[0] + " stages"
                r = timed(ctx, want)
                assert r, (name, want)
                print(f"{name}: repeat {rep}, {tag}: " + ", ".join(f"{k} {v:.3f} ms" for k, v in r.items()), flush=True)
                res[tag].append(r)
        for k in env:
            os.environ.pop(k, None)
        for kern in sorted(res[other][0]):
            p = np.array([r[kern] for r in res[other]])
            q = np.array([r[kern] for r in res["this tree"]])
            print(f"SUMMARY {name} ({stages}), {kern}: {other} mean {p.mean():.3f} ms (min {p.min():.3f}, max {p.max():.3f}, spread "
                  f"{p.max() - p.min():.3f}); this tree mean {q.mean():.3f} ms (min {q.min():.3f}, max {q.max():.3f}); this tree / {other} "
                  f"{q.mean() / p.mean():.4f}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
