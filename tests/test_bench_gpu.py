"""bench.py's input options on the GPU (the default synthetic run is what the driver times; this covers --images)."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_on_a_recorded_sequence_directory(tmp_path):
    """bench.py --images on a KITTI-shaped directory (times.txt, image_0/%06d.png, image_1/%06d.png -- Examples/PL/PL_stereo_kitti.cc:130-160 LoadImages): the image
    size comes from the files (here 600 x 368, none of the named configurations), the feature counts from --config, the JSON line is the synthetic run's."""
    import numpy as np
    from PIL import Image
    from orb_line_slam_amd import synth
    w, h, n = 600, 368, 6
    imgs = synth.stereo_batch(123, n, w, h)
    k = tmp_path / "kitti" / "07"
    (k / "image_0").mkdir(parents=True); (k / "image_1").mkdir()
    (k / "times.txt").write_text("".join("%e\n" % (0.1 * i) for i in range(n)))
    for i in range(n):
        Image.fromarray(imgs[2 * i]).save(k / "image_0" / ("%06d.png" % i))
        Image.fromarray(imgs[2 * i + 1]).save(k / "image_1" / ("%06d.png" % i))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--images", str(k), "--config", "C2", "--pairs", "8", "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--no-extras", "--no-isolated"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    d = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith("{")][0])
    assert d["data"] == "recorded: 07" and d["value"] > 0 and d["n_gpus"] == 1
    assert d["config"]["pairs_per_gpu_per_step"] == 8 and d["config"]["mean_keylines_per_image"] > 20


def _bench_line(cmd):
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_bench_dump_outputs(tmp_path):
    """bench.py --dump-outputs DIR: what the last timed step computed, as float32 / float64 .npy files of at most 64 MB in all -- the batch's
    counts and every output of a seeded sample of 16 pairs, rows past a frame's count zero -- identical from run to run with the same
    arguments; --steps sets the number of timed steps and ms_per_step is the time of one of them."""
    import numpy as np
    dumps = []
    for run in range(2):
        d_out = tmp_path / f"dump{run}"
        d = _bench_line([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C2", "--pairs", "24", "--distinct", "24", "--steps", "3", "--warmup", "1",
                         "--dump-outputs", str(d_out)])
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and abs(d["value"] - 24 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-3
        assert "cpu_baseline" not in d and "pair_latency_ms" not in d and "stages" not in d["roofline"]      # the legs of --full
        f = {p.stem: np.load(p) for p in d_out.glob("*.npy")}
        assert all(a.dtype in (np.float32, np.float64) for a in f.values()) and sum(a.nbytes for a in f.values()) <= 64 << 20
        assert d["dump_outputs"]["arrays"] == len(f) and d["dump_outputs"]["pairs"] == 16
        sp = f["sample_pairs"].astype(np.int64)
        assert len(sp) == 16 and len(set(sp.tolist())) == 16 and sp.min() >= 0 and sp.max() < 24
        oc, lc = f["orb_counts"].astype(np.int64), f["line_counts"].astype(np.int64)
        assert len(oc) == 48 and abs(oc.mean() - d["config"]["mean_keypoints_per_image"]) < 0.051
        assert len(lc) == 48 and abs(lc.mean() - d["config"]["mean_keylines_per_image"]) < 0.051
        kp, kl = f["keypoints"], f["keylines"]
        cap, lcap = kp.shape[1], kl.shape[1]
        assert kp.shape == (32, cap, 7) and f["descriptors"].shape == (32, cap, 32) and kl.shape == (32, lcap, 17)
        assert f["mvuRight"].shape == (16, cap) and f["line_matches_12"].shape == (16, lcap) and f["mvle_l"].shape == (16, lcap, 3)
        n_img = oc[np.stack([2 * sp, 2 * sp + 1], 1).reshape(-1)]
        for i in range(32):
            assert not kp[i, n_img[i]:].any() and (kp[i, :n_img[i], 0] >= 0).all() and (kp[i, :n_img[i], 0] < 640).all()
        # (matches of frame p + 1 against frame p, for the sampled p < 23; SearchByBoW's count per pair for the whole batch)
        assert f["f2f_orb_matches"].shape == ((sp < 23).sum(), cap) and f["f2f_orb_nmatches"].shape == (23,)
        assert (f["mvuRight"] > 0).any() and (f["mvDisparity_l"] > 0).any()      # stereo points and stereo lines were found
        dumps.append(f)
    assert dumps[0].keys() == dumps[1].keys() and all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])
