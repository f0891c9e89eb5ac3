"""The text hand-over of the report seams (texts_hand_over, sweepga_amd/csrc/host/host_internal.h) without a GPU and without
the library: tests/native/text_hand_over_check.cpp hands texts over under every pattern of wanted slots -- {1,0}, {0,1}, {1,1},
three slots {0,1,1} -- and checks that a wanted slot holds its text in a buffer of its own, NUL-terminated at its length (an
empty text: one NUL byte, length 0), and that an unwanted slot is left as the caller had it."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_texts_hand_over(tmp_path):
    exe = str(tmp_path / "text_hand_over_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "text_hand_over_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"ok": True, "failures": 0}
