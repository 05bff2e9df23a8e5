"""The packed launch slots of the quad kernel under ASan + UBSan: the stride / offset arithmetic of
pylda_amd/csrc/host_plan.cpp (quad_slot_layout) and the shared slot -> term mapping of estep_limits.h, compiled with plain
g++ together with tests/native/quad_slots_fuzz.cpp and run on random CSR corpora on the CPU - every (launch slot, word
group, word slot) holds the term id the kernel's own expression picks, -1 beyond the document, no two slots overlap and
the bytes are what Corpus.layout("quad_slot_bytes") reports."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quad_slot_arithmetic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "quad_slots_fuzz")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "pylda_amd", "csrc", "host_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "quad_slots_fuzz.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed: " + build.stderr.splitlines()[0])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, "150"], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "quad slots sanitizer run: ok" in run.stdout
