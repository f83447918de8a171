"""The two headers the passes over the vote's outputs share (csrc/bsdc_ssrows.h: the consensus-row
views, the duplex column rule and the per-read rate of DESIGN.md 3.8; csrc/bsdc_devtext.h: load4, can4
and the record writer) under the sanitizers as a stand-alone program.  No GPU: the device sides are
checked byte for byte against the host encoder, the twins and the numpy restatements by the passes'
own tests."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_shared_headers_under_sanitizers(tmp_path):
    """tests/sanitize/shared_headers_main.cpp: plain g++, -Wall -Werror, ASan and UBSan (host code, its own main)."""
    exe = str(tmp_path / "shared_headers")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "sanitize", "shared_headers_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shared headers ok" in r.stdout
