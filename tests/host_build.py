"""The one build of a host-mirror binary: tests/host_cpp/<driver>.cpp + racing-slam_amd/host/slam_host.cpp, linked against
librsgpu.so (and the oracle when the driver checks against it), rebuilt when anything it is made from is newer."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(ROOT, "racing-slam_amd")
ORACLE = os.path.join(ROOT, "oracle")


def build_host_binary(rs, driver, oracle=None, extra_srcs=()):
    """Path of tests/host_cpp/<driver>.bin, built with hipcc if stale."""
    rs.load()
    if oracle is not None:
        oracle.lib()
    exe = os.path.join(ROOT, "tests", "host_cpp", driver + ".bin")
    srcs = [os.path.join(ROOT, "tests", "host_cpp", driver + ".cpp"), os.path.join(AMD, "host", "slam_host.cpp")] + list(extra_srcs)
    # everything slam_host.cpp includes belongs here: a header missing from this list lets a stale binary pass the suite
    deps = srcs + [os.path.join(AMD, "host", "slam_host.h"), os.path.join(ROOT, "integration", "reference_shim", "rs_marshal.h"),
                   os.path.join(ROOT, "include", "rsgpu.h"), os.path.join(AMD, "librsgpu.so")]
    libs, rpaths = ["-L" + AMD, "-lrsgpu"], ["-Wl,-rpath," + AMD]
    if oracle is not None:
        deps.append(os.path.join(ORACLE, "liboracle.so"))
        libs += ["-L" + ORACLE, "-loracle"]
        rpaths.append("-Wl,-rpath," + ORACLE)
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-Wall", "-o", exe] + srcs + libs + rpaths + ["-lm"])
    return exe
