"""racing-slam_amd/csrc/carve.h on its own: tests/host_cpp/test_carve.cpp runs one layout on a null carver and on a malloc'ed
block and checks sizes, alignment, order, disjointness and every byte of every piece, as a stand-alone program (no GPU, no
librsgpu) under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carve_header_under_address_sanitizer():
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the sanitizer program"
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_carve.bin")
    src = os.path.join(ROOT, "tests", "host_cpp", "test_carve.cpp")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "carve checks passed" in r.stdout
