"""tools/compressor_probe.py — what DynamicsCompressorNode costs on the device (GPU box; bench.py does not know the node).

1024 contexts x 10 s at 48 kHz, a device-resident source (C2's footprint) -> compressor -> destination, mono and stereo, and C2
(source -> Biquad -> Gain -> destination, bench.py's builder) built and timed IN THE SAME PROCESS as the yardstick: 5 warm-up and
20 timed renders each, wall time per render between synchronisations and per-kernel times from the library's profile slots.

Derived figures: the level and apply kernels as a fraction of the same-process C2 rate PER BYTE MOVED (planes of n_contexts x
frames x 4 bytes: level reads nch and writes 1, apply reads 1 + nch and writes nch; C2 reads 2 and writes 2), and the detector in
cycles per sample per wavefront (time x clock / frames) — every wavefront walks the whole render, so the number does not depend on
the batch size until the wavefronts outnumber the SIMDs.

    python tools/compressor_probe.py [--instances 1024] [--seconds 10] [--out profiles/compressor_probe.json]

--meter: what the reduction trace costs (DynamicsCompressorNode(meter=True): a fourth launch, compressor_meter_kernel).  Per channel
count two batches, meter off and meter on, built in the same process and timed ALTERNATELY (off, on, off, on, ...: ROUNDS rounds of
the protocol above each), so that the meter-off leg is the comparison and not an earlier file's number; the meter-off wall time is
also set against the spread of profiles/compressor_probe.json and a difference beyond it is reported as it is.

    python tools/compressor_probe.py --meter [--out profiles/compressor_reduction_probe.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import web_audio_api_rs_amd as waa  # noqa: E402

SR = 48000.0
WARMUP, STEPS = 5, 20


def timed(ctx):
    """(wall ms per render, {kernel: ms per render})"""
    ctx.prepare()
    ctx.render_async()  # (plans, allocates, renders once)
    ctx.sync()
    for _ in range(WARMUP):
        ctx.render_async()
    ctx.sync()
    walls = []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        ctx.render_async()
        ctx.sync()
        walls.append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(STEPS):
        ctx.render_async()
    ctx.sync()
    kernels = {name: ms / STEPS for name, launches, ms in ctx.profile_entries() if launches}
    ctx.profile(False)
    walls.sort()
    return dict(wall_ms_median=walls[len(walls) // 2], wall_ms_min=walls[0], wall_ms_max=walls[-1], kernels_ms=kernels)


def compressor(hip, noise, n_inst, frames, n_ch, meter=False):
    ctx = waa.OfflineAudioContext(n_ch, frames, SR, n_instances=n_inst, binding=hip, device=0)
    src = ctx.create_buffer_source()
    src.adopt_device_buffer(noise.data_ptr(), n_ch, frames, SR)
    src.connect(ctx.create_dynamics_compressor(meter=meter)).connect(ctx.destination())
    src.start()
    return ctx


ROUNDS = 3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def meter_leg(hip, rec, noises, n, frames):
    """meter off / meter on, alternately, per channel count; rec["lines"]: one entry per channel count"""
    parent_path = os.path.join(ROOT, "profiles", "compressor_probe.json")
    parent = {l["channels"]: l for l in json.load(open(parent_path))["lines"]} if os.path.exists(parent_path) else {}
    for n_ch, noise in noises:
        legs = {False: compressor(hip, noise, n, frames, n_ch, False), True: compressor(hip, noise, n, frames, n_ch, True)}
        plan = [l for l in legs[True].plan_describe().splitlines() if l.startswith("compressor node")]
        rounds = {False: [], True: []}
        for _ in range(ROUNDS):
            for meter in (False, True):
                rounds[meter].append(timed(legs[meter]))
        for ctx in legs.values():
            ctx.close()
        off = median([r["wall_ms_median"] for r in rounds[False]])
        on = median([r["wall_ms_median"] for r in rounds[True]])
        meter_ms = median([r["kernels_ms"]["compressor_meter_kernel"] for r in rounds[True]])
        assert all("compressor_meter_kernel" not in r["kernels_ms"] for r in rounds[False])
        line = dict(channels=n_ch, plan=plan, rounds=ROUNDS, meter_kernel_ms=meter_ms, wall_ms_meter_off=off, wall_ms_meter_on=on,
                    wall_ms_difference=on - off, kernels_total_ms_meter_off=median([sum(r["kernels_ms"].values()) for r in rounds[False]]),
                    kernels_total_ms_meter_on=median([sum(r["kernels_ms"].values()) for r in rounds[True]]),
                    trace_values=n * (frames // 128), trace_mb=n * (frames // 128) * 4 / 1e6,
                    meter_off_rounds=rounds[False], meter_on_rounds=rounds[True])
        if n_ch in parent and n == 1024 and frames == 480000:
            p = parent[n_ch]
            line["parent_probe"] = dict(wall_ms_median=p["wall_ms_median"], wall_ms_min=p["wall_ms_min"], wall_ms_max=p["wall_ms_max"],
                                        meter_off_within_its_spread=bool(p["wall_ms_min"] <= off <= p["wall_ms_max"]),
                                        meter_off_minus_its_median_ms=off - p["wall_ms_median"])
        rec["lines"].append(line)
        print(f"compressor {n_ch}ch: meter off {off:.3f} ms | meter on {on:.3f} ms ({on - off:+.3f}) | compressor_meter_kernel {meter_ms:.4f} ms"
              + (f" | parent probe {line['parent_probe']['wall_ms_median']:.3f} ms [{line['parent_probe']['wall_ms_min']:.3f}, "
                 f"{line['parent_probe']['wall_ms_max']:.3f}]: meter off {'inside' if line['parent_probe']['meter_off_within_its_spread'] else 'OUTSIDE'} its spread"
                 if "parent_probe" in line else ""), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="engine clock if torch does not report one (MI355X: 2400)")
    ap.add_argument("--meter", action="store_true", help="the reduction trace: meter off / meter on alternately (see above)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "compressor_reduction_probe.json" if args.meter else "compressor_probe.json")
    n, frames = args.instances, int(args.seconds * SR) // 128 * 128
    hip = waa.default_binding()
    props = torch.cuda.get_device_properties(0)
    # (the device's peak engine clock where torch reports it, else --clock-mhz: the detector figure is time x clock / frames)
    clock_mhz = props.clock_rate / 1e3 if getattr(props, "clock_rate", 0) else args.clock_mhz
    plane_gb = n * frames * 4 / 1e9
    stereo = torch.empty((n, 2, frames), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    mono = torch.empty((n, 1, frames), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    torch.cuda.synchronize()
    rec = dict(instances=n, frames=frames, sample_rate=SR, warmup=WARMUP, steps=STEPS, plane_gb=plane_gb,
               device=torch.cuda.get_device_name(0), clock_mhz=clock_mhz, lines=[])
    if args.meter:
        meter_leg(hip, rec, ((1, mono), (2, stereo)), n, frames)
        write(rec, args.out)
        return
    c2, _ = bench.build_workload(waa, hip, "c2", n, frames, 0, stereo.data_ptr())
    t_c2 = timed(c2)
    c2.close()
    c2_ms = sum(t_c2["kernels_ms"].values())
    c2_gb_per_ms = 4 * plane_gb / c2_ms  # reads 2 planes, writes 2
    rec["c2"] = dict(t_c2, kernels_total_ms=c2_ms, planes_moved=4, gb_per_ms=c2_gb_per_ms)
    print(f"C2 (same process): wall {t_c2['wall_ms_median']:.3f} ms, kernels {c2_ms:.3f} ms = {c2_gb_per_ms * 1e3:.0f} GB/s", flush=True)
    for n_ch, noise in ((1, mono), (2, stereo)):
        ctx = compressor(hip, noise, n, frames, n_ch)
        plan = [l for l in ctx.plan_describe().splitlines() if l.startswith(("compressor node", "source node", "alias", "chain"))]
        t = timed(ctx)
        ctx.close()
        k = t["kernels_ms"]
        level, det, apply_ = k["compressor_level_kernel"], k["compressor_detector_kernel"], k["compressor_apply_kernel"]
        line = dict(t, channels=n_ch, plan=plan, kernels_total_ms=sum(k.values()),
                    level=dict(ms=level, planes_moved=n_ch + 1, fraction_of_c2_rate_per_byte=((n_ch + 1) * plane_gb / level) / c2_gb_per_ms),
                    apply=dict(ms=apply_, planes_moved=1 + 2 * n_ch, fraction_of_c2_rate_per_byte=((1 + 2 * n_ch) * plane_gb / apply_) / c2_gb_per_ms),
                    detector=dict(ms=det, wavefronts=(n + 63) // 64, ns_per_sample=det * 1e6 / frames,
                                  cycles_per_sample_per_wavefront=det * 1e-3 * clock_mhz * 1e6 / frames))
        rec["lines"].append(line)
        print(f"compressor {n_ch}ch: wall {t['wall_ms_median']:.3f} ms | level {level:.3f} ms ({line['level']['fraction_of_c2_rate_per_byte']:.2f} of C2's rate "
              f"per byte) | detector {det:.3f} ms ({line['detector']['ns_per_sample']:.2f} ns / sample"
              + f", {line['detector']['cycles_per_sample_per_wavefront']:.1f} cycles at {clock_mhz:.0f} MHz"
              + f") | apply {apply_:.3f} ms ({line['apply']['fraction_of_c2_rate_per_byte']:.2f})", flush=True)
    write(rec, args.out)


def write(rec, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
