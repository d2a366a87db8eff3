"""bench.py's command line: a plain run prints the headline line only; --full adds the measurements and checks behind it."""
import json
import os
import subprocess
import sys

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("roofline", "stages", "video_branch", "configs", "quality", "cpu_baseline")      # + every roofline_* key


def _parse(argv):
    old = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        return bench.parse()
    finally:
        sys.argv = old


def _extras(line):
    return sorted(k for k in line if k in EXTRAS or k.startswith("roofline_"))


def test_full_is_opt_in():
    assert not _parse([]).full
    assert not _parse(["--no-roofline"]).full
    a = _parse(["--full", "--no-cpu-baseline", "--no-quality", "--no-roofline", "--no-video-record", "--no-config-records"])
    assert a.full and a.no_cpu_baseline and a.no_quality and a.no_roofline and a.no_video_record and a.no_config_records


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(cuda, tmp_path):
    """C1's clip (8 x 512^2, Te = 8), one warm-up and one timed step, each run in a process of its own."""
    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--frames", "8", "--te", "8", "--src", "512", "--steps", "1", "--warmup", "1",
                            *extra], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    plain = run("--dump-outputs", str(tmp_path / "dump"))
    assert _extras(plain) == []
    assert plain["steps"] == 1 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["unit"] == "frames/sec"
    assert sorted(os.listdir(tmp_path / "dump")) == sorted(n + ".npy" for n in plain["dumped_outputs"]["shapes"])
    full = run("--full", "--no-cpu-baseline", "--no-quality")
    assert {"roofline", "stages", "video_branch", "roofline_mask_decoder_c4clip"} <= set(_extras(full))
    assert "quality" not in full and "cpu_baseline" not in full and "configs" not in full      # (configs: C2 only)
    keys = ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config")
    assert {k: full[k] for k in keys} == {k: plain[k] for k in keys}
