"""racing-slam_amd/csrc/ba_blocks.h on its own: tests/host_cpp/test_ba_blocks.cpp runs the workspace and pinned layouts of a
bundle-adjustment window and refine_pose's two blocks on a null carver and on malloc'ed blocks, over a grid of window sizes
and every flag combination, as a stand-alone program (no GPU, no HIP call, no librsgpu).  The header includes the kernels'
shared definitions, so hipcc builds it; the host side runs under the address and undefined-behaviour sanitizers.
Also: the windows tests/test_gpu_ba_blocks.py solves at the blocks' boundaries (tests/ba_block_cases.py), on the oracle alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ba_block_cases as BB
import ba_cases as B
import ba_compare as CMP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ba_block_layouts_under_address_sanitizer():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed to build the sanitizer program"
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_ba_blocks.bin")
    src = os.path.join(ROOT, "tests", "host_cpp", "test_ba_blocks.cpp")
    # host side only: the program launches nothing, so no device code is compiled into it
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Wall",
                           "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "BA block checks passed (288 windows, 96 pinned blocks)" in r.stdout


# ---- the windows tests/test_gpu_ba_blocks.py compares with the oracle (tests/ba_block_cases.py), on the oracle alone
WINDOWS = [(name, kw, opt, expect) for name, (kw, opt, expect) in BB.SINGLE.items()] + \
          [("batch%d" % i, kw, {}, None) for i, kw in enumerate(BB.BATCH)]


@pytest.mark.parametrize("name,kw,opt,expect", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_block_windows_end_as_stated_and_stably(oracle, synth, name, kw, opt, expect):
    """Each window ends usable, at the stated termination where one is stated, with a record of exactly `iterations`
    entries; and with the input points scaled by 1 +- 1e-13 the oracle repeats its schedule and moves its results by at
    most a tenth of the GPU comparison's tolerances (the rule of tests/test_ba_cases_cpu.py)."""
    w = synth.make_ba_window(**kw)
    c, p, s, tr = B.solve_oracle(oracle, w, opt)
    assert s["usable"] == 1 and len(tr) == s["iterations"] <= opt.get("max_num_iterations", 10)
    if expect is not None:
        assert s["termination"] == expect and s["iterations"] == opt["max_num_iterations"]
    for seed in (0, 1):
        sign = np.random.default_rng(seed).choice([-1.0, 1.0], w["points"].shape)
        pc, pp, ps, ptr = B.solve_oracle(oracle, dict(w, points=w["points"] * (1.0 + 1e-13 * sign)), opt)
        CMP.assert_same_solve(dict(s=ps, tr=ptr, c=pc, p=pp), (c, p, None, None, s, tr), scale=0.1, initial=False)


def test_batch_windows_differ(oracle, synth):
    ws = [synth.make_ba_window(**kw) for kw in BB.BATCH]
    assert len({len(w["cams"]) for w in ws}) == len({len(w["points"]) for w in ws}) == len(ws) and max(len(w["cams"]) for w in ws) == 64
    assert all(int(np.sum(w["cam_free"])) <= 21 for w in ws)
    assert len({B.solve_oracle(oracle, w, {})[2]["iterations"] for w in ws}) >= 2
