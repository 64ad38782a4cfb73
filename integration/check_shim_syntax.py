#!/usr/bin/env python3
"""Front-end (-fsyntax-only) check of the drop-in translation units in integration/reference_shim/.

    python integration/check_shim_syntax.py <Racing-SLAM checkout>/src

The shims are OUR marshalling code, but they include the upstream project's own headers and Eigen / OpenCV.  This
type-checks them against the upstream project's REAL headers (the directory given) with the minimal Eigen / OpenCV
stand-ins of tests/shim_stubs/ (declarations only; see its README: this is not a build of the upstream project — none
of its .cpp files is compiled, nothing is linked or run, no parity claim rests on it).  It catches a missing
definition, helpers that do not exist, and signatures that drifted from the headers.  The upstream headers are not
part of this repository, so this is a maintainer's tool and not part of the test suite (tests/test_shim_syntax.py
keeps the checks that need only this repository).  Exit status 0: every unit type-checks.
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "integration", "reference_shim")
UNITS = ("MapMatcher.cpp", "Triangulation.cpp", "Optimization.cpp", "LocalWindow.cpp")


def flags(upstream_src):
    return ["-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-Wno-reorder",
            "-I" + os.path.join(ROOT, "tests", "shim_stubs"), "-I" + upstream_src, "-I" + os.path.join(ROOT, "include"),
            "-I" + SHIM]


def check(path, upstream_src):
    """(ok, compiler diagnostics) of one translation unit."""
    cxx = shutil.which("g++") or shutil.which("c++")
    r = subprocess.run([cxx] + flags(upstream_src) + [path], capture_output=True, text=True)
    return r.returncode == 0, r.stderr


# The two optional caller edits (.inc), spliced into skeletons of the functions they belong to (kept head / tail of
# the upstream function reduced to the declarations the block relies on).
INC_HARNESS = r'''
#include <algorithm>
#include <iostream>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include "Mapper.h"
#include "Frame.h"
#include "Map.h"
#include "MapPoint.h"
#include "TrackStore.h"
#include "Trajectory.h"
#include "rs_shim_common.h"
namespace slam {
namespace {
// the constants of src/Mapper.cpp:21-39 that the .inc files use (values as in the reference)
constexpr size_t MIN_NEW_POINTS_PER_KEY_FRAME = 100;
constexpr float ANY_PARALLAX_COSINE = 1.0F;
constexpr float TRACK_MAX_REPROJECTION_ERROR = 4.0F;
constexpr float TRACK_MIN_PARALLAX_COSINE = 0.999848F;
constexpr float ROTATION_PARALLAX_FACTOR = 0.20F;
constexpr float MAX_POINT_REPROJECTION_ERROR = 3.0F;
}
void Mapper::triangulate_tracks(KeyFrame& key_frame, TrackStore& tracks, const Trajectory& trajectory, FrameDiagnostics& diagnostics)
{
    struct Candidate { const Track* track; Eigen::Vector3f position; size_t keypoint_index; float parallax_cosine; float required_cosine; };
    std::vector<Candidate> candidates;
    std::vector<TrackId> inconsistent;
#include "Mapper_triangulate_tracks.inc"
    for (size_t index : accepted) { const auto& candidate = candidates[index]; (void)candidate.track->sightings.size(); }
    (void)topped_up;
}
void Mapper::cull_points(FrameDiagnostics& diagnostics, KeyFrame& key_frame)
{
    std::unordered_set<MapPoint*> local;
#include "Mapper_cull_points.inc"
    for (const auto& point : points_to_remove) m_map.remove_point(point);
}
}  // namespace slam
'''


def main(argv):
    if len(argv) != 2 or not os.path.isfile(os.path.join(argv[1], "MapMatcher.h")):
        sys.exit("usage: check_shim_syntax.py <Racing-SLAM checkout>/src  (the directory holding MapMatcher.h)")
    upstream_src = os.path.abspath(argv[1])
    failed = []
    with tempfile.TemporaryDirectory() as d:
        harness = os.path.join(d, "inc_harness.cpp")
        with open(harness, "w") as fh:
            fh.write(INC_HARNESS)
        for name, path in [(u, os.path.join(SHIM, u)) for u in UNITS] + [("Mapper .inc harness", harness)]:
            ok, err = check(path, upstream_src)
            print("%-22s %s" % (name, "ok" if ok else "FAILED"))
            if not ok:
                print(err[-4000:])
                failed.append(name)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main(sys.argv)
