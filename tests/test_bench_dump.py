"""bench.py --dump-outputs / --full: what a plain run writes of its last step, on the CPU oracle (the writer only needs a rendered
batch: the same ABI on either library).  CPU only; the bench run itself needs a GPU."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import web_audio_api_rs_amd as waa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("waa_bench_dump_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rendered(orc, n_inst=12, frames=128 * 9 + 5):
    noise = np.random.default_rng(7).uniform(-1.0, 1.0, (n_inst, 2, frames)).astype(np.float32)
    ctx = waa.OfflineAudioContext(2, frames, 48000.0, n_instances=n_inst, binding=orc)
    src = ctx.create_buffer_source()
    src.set_buffer_batch(noise, 48000.0)
    src.connect(ctx.create_biquad_filter(type_="lowpass", frequency=200.0, q=1.0)).connect(ctx.create_gain(gain=0.5)).connect(ctx.destination())
    src.start()
    ctx.render_async()
    ctx.sync()
    full = np.empty((n_inst, 2, frames), np.float32)
    orc.check(orc.download_all(ctx._handle, full.ctypes.data_as(waa.api._FP)))
    return ctx, full


def test_whole_batch_when_it_fits(bench, orc, tmp_path):
    ctx, full = _rendered(orc)
    bench.dump_outputs(ctx, str(tmp_path))
    ctx.close()
    assert sorted(os.listdir(tmp_path)) == ["output.npy"]
    out = np.load(tmp_path / "output.npy")
    assert out.dtype == np.float32 and np.array_equal(out, full)


def test_seeded_sample_under_the_budget(bench, orc, tmp_path, monkeypatch):
    ctx, full = _rendered(orc)
    frames = full.shape[2]
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096 + 5 * 2 * frames * 4 + 100)  # room for 5 of the 12 contexts
    bins = np.arange(12 * 8, dtype=np.float32).reshape(12, 8)
    bench.dump_outputs(ctx, str(tmp_path / "a"), bins)
    bench.dump_outputs(ctx, str(tmp_path / "b"), bins)
    ctx.close()
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BYTES
    a, b = np.load(tmp_path / "a" / "output.npy"), np.load(tmp_path / "b" / "output.npy")
    assert np.array_equal(a, b)  # fixed seed: the same contexts every time
    assert a.shape[1:] == (2, frames) and 1 <= a.shape[0] < 12
    rows = [next(i for i in range(12) if np.array_equal(full[i], a[j])) for j in range(a.shape[0])]
    assert rows == sorted(set(rows))
    assert np.array_equal(np.load(tmp_path / "a" / "analyser_db.npy"), bins[rows])  # the same contexts' analyser rows


def test_frames_are_sampled_when_one_context_is_too_large(bench, orc, tmp_path, monkeypatch):
    ctx, full = _rendered(orc, n_inst=3)
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096 + 2 * 300 * 4)
    bench.dump_outputs(ctx, str(tmp_path))
    ctx.close()
    out = np.load(tmp_path / "output.npy")
    assert out.shape == (1, 2, 300) and os.path.getsize(tmp_path / "output.npy") <= bench.DUMP_BYTES
    # the sampled frames are, in order, frames of one rendered context
    row = next(i for i in range(3) if np.isin(out[0, 0], full[i, 0]).all())
    assert np.isin(out[0, 1], full[row, 1]).all()


def test_the_options_exist():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
