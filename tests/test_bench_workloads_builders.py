"""CPU side of tests/test_bench_workloads_full_size.py: the graph the -m gpu module compares with the oracle is the graph bench.py
times, and every bench workload has a full-size every-instance test.

The oracle renders bench.build_workload's batch unchunked and through the test's chunked builder (the fix-ups of
tests/bench_workloads.py re-apply the values bench sets by instance index and count); the two must be bit-identical.  128
contexts, chunks 0..48 and 48..128: the oscillator's detune stride (n // 64) is 2 for the batch and 1 for both chunks, the
per-context HRTF positions are counted from 48 in the second chunk."""
import os

import numpy as np
import pytest

import web_audio_api_rs_amd as waa
from bench_workloads import ELSEWHERE, HRTF_PER_CONTEXT, SR, WORKLOADS, load_bench, oracle_builder
from graphs import assert_all_finite

N_INST, FRAMES = 128, 128 * 40 + 37
CHUNKS = ((0, 48), (48, 128))


@pytest.fixture(scope="module")
def bench():
    return load_bench()


def _render(ctx):
    out = ctx.start_rendering_sync().data
    ctx.close()
    return out


@pytest.mark.parametrize("name,per_context", [(n, False) for n in sorted(WORKLOADS)] + [("hrtf", True)])
def test_chunked_oracle_builder_is_the_bench_graph(bench, orc, name, per_context, monkeypatch):
    if per_context:
        monkeypatch.setenv(HRTF_PER_CONTEXT, "1")
    else:
        monkeypatch.delenv(HRTF_PER_CONTEXT, raising=False)
    rng = np.random.default_rng(0xBE1C)
    noise = rng.uniform(-1.0, 1.0, (N_INST, 2, FRAMES)).astype(np.float32) if WORKLOADS[name].has_input else None
    ctx, src = bench.build_workload(waa, orc, name, N_INST, FRAMES, 0, None)
    if noise is not None:
        src.set_buffer_batch(noise, SR)
    whole = _render(ctx)
    assert_all_finite(whole, f"{name}: the unchunked render")
    assert np.abs(whole).max() > 1e-3
    build = oracle_builder(bench, name, noise, N_INST, FRAMES)
    for lo, hi in CHUNKS:
        ctx, _ = build(orc, lo, hi)
        part = _render(ctx)
        same = part.view(np.uint32) == whole[lo:hi].view(np.uint32)
        assert same.all(), f"{name}: chunk {lo}..{hi} differs from bench's batch first at {np.argwhere(~same)[0] + [lo, 0, 0]}"
    if name == "osc" or per_context:
        # the fix-ups matter: the contexts really differ by index (else this test could not see a wrong fix-up)
        assert not np.array_equal(whole[0], whole[2]) and not np.array_equal(whole[1], whole[2])


def test_every_bench_workload_has_a_full_size_parity_test(bench):
    """a workload added to bench.py without a parity test at its benchmarked size fails here"""
    choices = set(bench.ALG_BYTES)  # bench.py's --workload choices
    assert not set(WORKLOADS) & set(ELSEWHERE)
    missing = choices - set(WORKLOADS) - set(ELSEWHERE)
    assert not missing, f"bench.py workloads without a full-size every-instance test: {sorted(missing)}"
    assert set(WORKLOADS) | set(ELSEWHERE) <= choices, "the tables name a workload bench.py no longer has"
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_full_size_all_instances.py")).read()
    for name, test in ELSEWHERE.items():
        assert f"def {test}(" in src, (name, test)
