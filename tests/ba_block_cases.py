"""Windows at the boundaries of the bundle-adjustment driver's per-call blocks (csrc/ba_blocks.h), shared by
tests/test_ba_blocks_cpu.py (the oracle ends every one as stated here, stably) and tests/test_gpu_ba_blocks.py (the GPU
against the oracle).

  SINGLE   name -> (make_ba_window arguments, rs_ba_options fields, termination the oracle must reach or None: any usable end)
           64 key frames: the last window whose free-camera table is the mask; 65: the first that uploads the slot and
           free-camera tables through the pinned block.  max_num_iterations 0 and 1 on the 3-camera window: a record of no
           and of one entry next to the camera mirror
  BATCH    windows of one rs_bundle_adjust_batch call in its grid form, default options: different camera and landmark
           counts, ending at different iterations.  The 64-camera window keeps 20 cameras free: 64 is the most the grid
           takes, and 21 free cameras the most its reduced solve holds
  INERTIAL the smallest consecutive-factor window of tests/inertial_cases.py, solved under both "ba_imu_mode" values
"""
from inertial_cases import NO_CONVERGENCE

_W3 = dict(n_kf=3, n_points=60, run_min=3, run_max=6)
# a chain of 62 / 63 free cameras held by 120 landmarks: after ten iterations 1e-13 on the input moves the result past the
# GPU comparison's tolerances, after four by less than a tenth of them (as ba_cases.CLASS_OPT has it for its 129-camera chain)
_CHAIN = dict(max_num_iterations=4)
SINGLE = {
    "kf3": (dict(_W3, config_id=301), {}, None),
    "kf64": (dict(n_kf=64, n_points=120, run_min=6, run_max=10, config_id=302), _CHAIN, NO_CONVERGENCE),
    "kf65": (dict(n_kf=65, n_points=120, run_min=6, run_max=10, config_id=302), _CHAIN, NO_CONVERGENCE),
    "kf3_max_iter_0": (dict(_W3, config_id=301), dict(max_num_iterations=0), NO_CONVERGENCE),
    "kf3_max_iter_1": (dict(_W3, config_id=301), dict(max_num_iterations=1), NO_CONVERGENCE),
}
BATCH = [dict(_W3, config_id=304), dict(n_kf=8, n_points=100, run_min=3, run_max=6, config_id=305),
         dict(n_kf=64, n_points=120, run_min=6, run_max=10, n_fixed=44, config_id=306)]
INERTIAL = "ci2_one_factor"
