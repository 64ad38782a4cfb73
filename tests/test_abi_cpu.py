"""CPU tests of the boundary: the C-ABI library loads, exports every symbol that
include/rsgpu.h declares, and refuses to compute without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rsgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(rs):
    lib = rs.load()
    syms = declared_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert sorted(rs.EXPORTS) == syms
    assert lib.rs_abi_version() == 3


def test_no_cpu_fallback(rs):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    rc = rs.load().rs_context_create(0, C.byref(h))
    assert rc == 6 and not h.value          # RS_ERR_NO_DEVICE
    with pytest.raises(rs.RsError):
        rs.Context(0)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "racing-slam_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "pyoracle" not in src and "liboracle" not in src and "rs_oracle.h" not in src, f


def test_default_options_match_oracle(rs, oracle):
    a, b = rs.default_options(), oracle.default_options()
    for name, _ in a._fields_:
        assert getattr(a, name) == getattr(b, name), name


def test_bench_metric_is_baseline_json_s_string():
    """The line bench.py prints must carry BASELINE.json's metric character for character (the driver matches on it)."""
    import json
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "BASELINE.json"), encoding="utf-8") as f:
        assert bench.METRIC == json.load(f)["metric"]
    assert bench.visible_gpu_count() >= 0        # sysfs / environment only: no HIP call


def test_bench_dump_outputs_writes_float_arrays(tmp_path):
    """bench.py --dump-outputs: one .npy per output of the pass, f32 kept, everything else widened to f64 exactly."""
    import numpy as np
    import bench
    i32 = np.array([3, 1, 2], np.int32)
    f32 = np.arange(6, dtype=np.float32).reshape(2, 3) + np.float32(0.1)
    got = dict(mq=i32, mt=i32, ra=dict(match_kp=i32, match_point=i32), rb=dict(match_kp=i32, match_point=i32),
               tri=dict(keep=np.array([1, 0], np.uint8), xyz=f32, out_index=i32),
               trk=dict(status=i32, xyz=f32, accepted=i32, inconsistent=i32, parallax_cos=f32[0], required_cos=f32[1]),
               lw=(i32, np.array([1, 0, 1], np.uint8)), cams=np.ones((4, 6)), pts=np.ones((5, 3)),
               ba=dict(termination=0, iterations=10, successful_steps=9, usable=1, initial_cost=2.5, final_cost=1.5, final_radius=1e4),
               after=np.ones((4, 16), np.float32), single=f32)
    bench.dump_outputs(str(tmp_path), got)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert len(names) == 22 and all(n.endswith(".npy") for n in names)
    for n in names:
        assert np.load(tmp_path / n).dtype in (np.float32, np.float64), n
    assert np.array_equal(np.load(tmp_path / "match_descriptors.query.npy"), i32.astype(np.float64))
    assert np.load(tmp_path / "triangulate.xyz.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "triangulate.xyz.npy"), f32)
    assert np.load(tmp_path / "bundle_adjust.summary.npy").tolist() == [0, 10, 9, 1, 2.5, 1.5, 1e4]
