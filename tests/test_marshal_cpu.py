"""integration/reference_shim/rs_marshal.h on its own: tests/host_cpp/test_marshal.cpp instantiates the flatten templates
and PtrIndex with a third set of plain structs and compares every output array with an obvious restatement, as a
stand-alone program (no GPU, no librsgpu) under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_marshal_header_under_address_sanitizer():
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the sanitizer program"
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_marshal.bin")
    # rs_pack_pose (flatten_ba's camera packing) is host code of the library: csrc/host.cpp, compiled in
    srcs = [os.path.join(ROOT, "tests", "host_cpp", "test_marshal.cpp"), os.path.join(ROOT, "racing-slam_amd", "csrc", "host.cpp")]
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread",
                           "-o", exe] + srcs + ["-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "marshal checks passed" in r.stdout
