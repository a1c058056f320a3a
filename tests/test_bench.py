"""The bench.py contract (the driver's BENCH line): one JSON line with the metric, the whole-job
value and the timing fields; with --full also the roofline and cpu_baseline objects, on the headline
workload. A plain run does nothing but its timed steps and can write their film (--dump-outputs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1",
                        "--cpu-seconds", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "roofline_shade", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["config"]["workload"].startswith("C3: synth-1M, 1024x1024, 64 spp")
    # value = traced rays per second over the timed steps; the reference-equivalent count beside it
    assert abs(d["value"] - d["rays_traced_per_path"] * 1024 * 1024 * 64 / (d["ms_per_step"] * 1e-3) / 1e6) < 0.01 * d["value"]
    assert d["value"] == d["mrays_traced_per_s"]
    assert abs(d["mrays_reference_equivalent_per_s"] - d["rays_per_path"] * 1024 * 1024 * 64
               / (d["ms_per_step"] * 1e-3) / 1e6) < 0.01 * d["value"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert 0.25 < rf["frac"] <= 1.05 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 0.01
    assert rf["peak"] == 34500.0 and rf["unit"] == "GB/s"  # a hardware peak (MI355X aggregate L2)
    # the drop-in frame loop: 1-spp calls, films bit-identical to the batched render
    di = d["dropin"]
    for pol in ("queued", "sync", "sync_read"):
        assert di[pol]["film_equals_batched"] is True and di[pol]["ms_per_frame"] > 0, pol
    assert di["queued"]["ms_per_frame"] <= di["sync_read"]["ms_per_frame"]
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] in ("reference", "port") and cb["value"] > 0


HEADLINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config")
FULL_ONLY_KEYS = ("roofline", "roofline_shade", "cpu_baseline", "dropin", "kernel_timing", "kernel_ms_per_step_rank0")


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_film(tmp_path):
    """Without --full the line holds the headline fields and none of the other legs' objects, and
    --dump-outputs writes the film the timed steps left (3 queued 4-spp renders adding into a film
    cleared once: 12 spp), identical from run to run and equal to one render of the same samples."""
    import numpy as np
    from raytracingrenderer_amd import RayTracer, loadScene
    films = []
    for run in ("a", "b"):
        out = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--config", "C2", "--width", "96", "--height", "64", "--spp", "4",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 1
        d = json.loads(lines[0])
        for k in HEADLINE_KEYS:
            assert k in d, k
        for k in FULL_ONLY_KEYS:
            assert k not in d, k
        assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert d["unit"] == "Mray/s" and d["dtype"] == "f32" and d["higher_is_better"] is True
        assert abs(d["value"] - d["rays_traced_per_path"] * 96 * 64 * 4 / (d["ms_per_step"] * 1e-3) / 1e6) < 0.01 * d["value"]
        assert sorted(os.listdir(out)) == ["film.npy", "film_nonfinite.npy", "spp.npy"]
        film, spp = np.load(out / "film.npy"), np.load(out / "spp.npy")
        assert film.dtype == np.float32 and film.shape == (64, 96, 3) and spp.dtype == np.float64
        assert spp.tolist() == [12.0]
        assert np.isfinite(film).all() and not np.load(out / "film_nonfinite.npy").any()
        films.append(film)
    assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32))
    # the same three renders through the library (bench.py's C2: cornell-box, depth 8, seed 1234)
    s = loadScene(os.path.join(ROOT, "tests", "golden", "scenes", "cornell-box"), width=96, height=64)
    rt = RayTracer(s, seed=1234, max_depth=8)
    for _ in range(3):
        rt.render(4, first_sample=0)
    assert np.array_equal(rt.film()[0].view(np.uint32), films[0].view(np.uint32))


def test_dump_outputs_samples_a_film_over_the_cap(tmp_path):
    """CPU: a film over the 64 MB cap is written as a fixed choice of pixels with their indices."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    h, w = 1800, 1600  # 35 MB of float32 RGB, 69 MB with the marks
    film = np.arange(h * w * 3, dtype=np.float32).reshape(h, w, 3)
    film[5, 7] = (np.nan, np.inf, -np.inf)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), film, 7)
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    b = {f: np.load(tmp_path / "b" / f) for f in sorted(os.listdir(tmp_path / "b"))}
    assert sorted(a) == ["film.npy", "film_nonfinite.npy", "film_pixels.npy", "spp.npy"] and sorted(b) == sorted(a)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= 64 << 20
    pix = a["film_pixels.npy"].astype(np.int64)
    assert a["film.npy"].dtype == np.float32 and a["film.npy"].shape == (len(pix), 3)
    assert len(np.unique(pix)) == len(pix) and 0 <= pix.min() and pix.max() < h * w
    want = film.reshape(-1, 3)[pix]
    assert np.isfinite(a["film.npy"]).all()
    assert np.array_equal(a["film.npy"], np.where(np.isfinite(want), want, 0))
    assert np.array_equal(a["film_nonfinite.npy"] != 0, ~np.isfinite(want))
    # a film under the cap keeps its shape, and its three kinds of non-finite values their marks
    bench.dump_outputs(str(tmp_path / "c"), film[:16, :16], 1)
    small, mark = np.load(tmp_path / "c" / "film.npy"), np.load(tmp_path / "c" / "film_nonfinite.npy")
    assert small.shape == mark.shape == (16, 16, 3) and mark.dtype == np.float32 and np.isfinite(small).all()
    assert mark[5, 7].tolist() == [1.0, 2.0, 3.0] and small[5, 7].tolist() == [0.0, 0.0, 0.0] and mark.sum() == 6.0
    assert np.array_equal(small[mark == 0], film[:16, :16][mark == 0])
    for f in a:
        assert np.array_equal(a[f], b[f]), f
    assert a["spp.npy"].tolist() == [7.0]


def test_verify_film_needs_full():
    """CPU: --verify-film is a --full leg; asking for it in a plain run is an argument error."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--devices", "0,0", "--verify-film"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr
