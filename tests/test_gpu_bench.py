"""`python bench.py --gpus 1 --steps K --warmup W` on a small ring: one JSON line with the headline keys and none of the --full
legs, and --dump-outputs writes the last timed pass's results -- the same K passes from the prior in a fresh context give them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("repeats", "settled_window", "roofline", "roofline_bruteforce", "cold_registration", "projected_scaling",
             "secondary_stress_36x1M", "secondary_sequential", "cpu_baseline", "cpu_baseline_openmp")


@pytest.mark.timeout(600)
def test_plain_bench_line_and_dumped_outputs(mvr, tmp_path):
    V, N, K, max_dist = 12, 20000, 3, 4.0
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1",
                        "--points", str(N), "--dump-outputs", str(out_dir)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == K and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "correspondences/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert not [k for k in FULL_ONLY if k in line]

    got = {f[:-len(".npy")]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert set(got) == {"poses", "pair_transforms", "pair_correspondences", "pair_mse", "lum_pose", "edge_table"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["poses"].shape == (V, 4, 4) and got["edge_table"].shape[0] == V

    sp = mvr.synth_params(V, 3)
    piv, ax = mvr.synth_prior(sp)
    poses0 = [np.eye(4)] + [mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, V)) for v in range(1, V)]
    with mvr.Context(0) as ctx:
        for v in range(V):
            ctx.upload(V + v, mvr.synth_view(sp, v, N))
        poses, info = ctx.ring_step(list(range(V)), [V + v for v in range(V)], [(i, (i + 1) % V) for i in range(V)], poses0,
                                    max_dist, np.array(sp.pivot), steps=K)
    assert np.array_equal(got["pair_correspondences"], np.asarray(info["pair_n"], np.float64))
    assert np.abs(got["poses"] - poses).max() < 1e-9
    np.testing.assert_allclose(got["edge_table"], info["rows"], rtol=1e-9, atol=1e-9)
