#!/usr/bin/env python
"""tools/ab_render_bits.py <other.so> — are the quantum-serial kernels (dyn_kernel, loop_kernel) of another build of the library
BIT-identical to this tree's?  Renders the tests' own small graphs with csrc/libwaa_hip_measure.so and with <other.so> (a
measurement build too: the switches below exist only there) in one process and requires np.array_equal:
  * the random graphs of tests/test_fuzz_graphs.py, seeds 300-419, both generators, whose plan has a pipelined dynamic-count group
    (the corpus of test_quantum_pipeline_is_bit_identical_to_the_one_wavefront_form) — as planned, with WAA_DYN_NO_PIPE=1 and with
    WAA_DYN_NO_SCAN=1;
  * g_loop_kernel / g_loop_kernel_shaper of tests/test_launch_list.py and a Delay <-> Biquad <-> Gain loop under WAA_LOOP_KERNEL=1;
  * one graph per wide instantiation of dyn_kernel, out of tests/test_wide_channels.py: sources of 6 / 8 / 16 / 32 channels whose plan
    names dyn_kernel.  (The plan text does not name the instantiation; the launcher picks it from the widest signal of the group,
    dyn_planes() of waa_internal.hpp, which maps these four widths to <6, 1>, <8, 1>, <16, 1> and <32, 1>.)
Prints the graphs compared per kernel form and fails if a form has none.  (GPU box)"""
import collections
import ctypes
import os
os.environ.setdefault("WAA_USE_MEASURE_LIB", "1")  # A/B and probe tools flip measurement switches: libwaa_hip_measure.so
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import web_audio_api_rs_amd as waa  # noqa: E402
import test_cycles  # noqa: E402
import test_launch_list  # noqa: E402
import test_wide_channels  # noqa: E402
from graphs import white_noise  # noqa: E402
from test_fuzz_graphs import build_random_graph  # noqa: E402

waa.set_hrtf_database(os.path.join(ROOT, "tests", "golden", "IRC_1003_C.bin"))

LOOP_NOTE = "feedback loop: "  # (the plan's note of a loop_kernel launch: "feedback loop: N item(s) per quantum [...]")
compared = collections.Counter()
refused = collections.Counter()
last_plan = [""]
_render = waa.OfflineAudioContext.start_rendering_sync


def _render_and_keep_the_plan(self):
    last_plan[0] = self.plan_describe()
    return _render(self)


waa.OfflineAudioContext.start_rendering_sync = _render_and_keep_the_plan


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k in self.kv:
            os.environ.pop(k, None)


def both(libs, form, render, must_name):
    """render(binding) -> samples, once per library; the plan must name the kernel the form is about"""
    outs = []
    for _, be in libs:
        outs.append(render(be))
        assert must_name in last_plan[0], (form, must_name, last_plan[0])
    a, b = (np.ascontiguousarray(o, dtype=np.float32).view(np.uint32) for o in outs)  # bit for bit: NaN payloads and signed zeros count
    if not np.array_equal(a, b):
        raise SystemExit(f"{form}: {libs[1][0]} differs from {libs[0][0]} in {int((a != b).sum())} sample(s), "
                         f"max |d| = {float(np.nanmax(np.abs(outs[0] - outs[1])))}")
    compared[form] += 1


def fuzz_render(seed, frozen):
    def go(be):
        ch, _ = build_random_graph(be, seed, frozen=frozen)
        out = ch.start_rendering_sync().data
        ch.close()
        return out
    return go


def main(argv):
    libs = [("this tree", waa.measure_binding()), (os.path.basename(argv[0]), waa.bind(ctypes.CDLL(os.path.abspath(argv[0])), "waa_"))]
    staged = set()
    for seed in range(300, 420):
        for frozen in (False, True):
            ch, _ = build_random_graph(libs[0][1], seed, frozen=frozen)
            try:
                plan = ch.plan_describe()
            except waa.WaaError as e:
                ch.close()
                if e.status != 4:
                    raise
                refused["random graphs"] += 1
                continue
            ch.close()
            if "pipelined over the quanta" not in plan:
                continue
            for line in plan.splitlines():
                if "pipelined over the quanta in" in line:
                    staged.add(int(line.split("pipelined over the quanta in ")[1].split()[0]))
            both(libs, "dyn_kernel<2, W > 1>, random graphs as planned", fuzz_render(seed, frozen), "pipelined over the quanta")
            with env(WAA_DYN_NO_PIPE="1"):
                both(libs, "dyn_kernel<2, 1>, the same with WAA_DYN_NO_PIPE=1", fuzz_render(seed, frozen), "dyn_kernel")
            with env(WAA_DYN_NO_SCAN="1"):
                both(libs, "dyn_kernel<2, W>, the same with WAA_DYN_NO_SCAN=1", fuzz_render(seed, frozen), "dyn_kernel")

    def launch_list_graph(builder):
        def go(be):
            c = builder(be)
            c.device = -1  # (the builders of the launch-list corpus make plan-only contexts)
            out = c.start_rendering_sync().data
            c.close()
            return out
        return go
    for builder in (test_launch_list.g_loop_kernel, test_launch_list.g_loop_kernel_shaper):
        both(libs, "loop_kernel, tests/test_launch_list.py", launch_list_graph(builder), LOOP_NOTE)
    noise = white_noise(5, 2, 2048 * 7 + 300, seed0=31)
    delays, gains = np.float32([0.0430, 0.05, 0.0861, 0.1, 0.0999]), np.float32([0.5, -0.7, 0.9, 0.3, 0.6])
    with env(WAA_LOOP_KERNEL="1"):
        for with_filter in (True, False):
            both(libs, "loop_kernel forced (WAA_LOOP_KERNEL=1), Delay <-> [Biquad ->] Gain",
                 lambda be: test_cycles._feedback_graph(be, noise, delays, gains, with_filter), LOOP_NOTE)
        with env(WAA_DYN_NO_SCAN="1"):
            both(libs, "loop_kernel forced, WAA_DYN_NO_SCAN=1", lambda be: test_cycles._feedback_graph(be, noise, delays, gains, True), LOOP_NOTE)
    for n in (6, 8, 16, 32):  # (the source of a wider bus ends early: a count change mid-render; 5.1 also around an echo loop with a filter)
        wide = [lambda be: test_wide_channels._ordered_sum(be, ["mono", "stereo", "wide"], n, n, stereo_frames=5 * test_wide_channels.RQ)[0]]
        if n == 6:
            wide.append(lambda be: test_wide_channels._echo_loop(be, 6, 0.004, True, True)[0])
        for render in wide:
            both(libs, f"dyn_kernel<{n}, 1> ({n}-channel sources), tests/test_wide_channels.py", render, "dyn_kernel")
    for form in sorted(compared):
        print(f"{compared[form]:4d} graph(s) bit-identical: {form}")
    for what in sorted(refused):
        print(f"{refused[what]:4d} refused by the planner (status 4), skipped: {what}")
    print(f"stage counts seen: {sorted(staged)}")
    forms = ["as planned", "WAA_DYN_NO_PIPE", "WAA_DYN_NO_SCAN=1", "test_launch_list", "loop_kernel forced (", "dyn_kernel<6,", "dyn_kernel<8,",
             "dyn_kernel<16,", "dyn_kernel<32,"]
    missing = [f for f in forms if not any(f in k for k in compared)]
    if missing:
        raise SystemExit(f"nothing compared for: {missing}")
    if compared["dyn_kernel<2, W > 1>, random graphs as planned"] < 20 or len(staged) < 2:
        raise SystemExit("fewer than 20 pipelined random graphs or fewer than two stage counts")
    print("all bit-identical")


if __name__ == "__main__":
    main(sys.argv[1:])
