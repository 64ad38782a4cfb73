"""Self-contained checks of the drop-in translation units in integration/reference_shim/.

Type-checking them needs the upstream project's own headers, which are not part of this repository: that check is
integration/check_shim_syntax.py, run by a maintainer against an upstream checkout.  What needs only this repository
stays here.
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "integration", "reference_shim")


def test_every_declared_function_of_the_four_headers_is_defined():
    """A drop-in must define every function the kept headers declare (r1: pose_graph was missing)."""
    text = "".join(open(os.path.join(SHIM, f)).read() for f in ("MapMatcher.cpp", "Triangulation.cpp", "Optimization.cpp", "LocalWindow.cpp"))
    for sym in ("MapMatcher::MapMatcher", "MapMatcher::match_map", "MapMatcher::match_key_frame", "MapMatcher::match_for_fuse",
                "MapMatcher::match_descriptors", "MapMatcher::match(", "get_matching_points(", "bool refine_pose(",
                "bool bundle_adjust(", "bool pose_graph(", "build_local_window("):
        assert sym in text, sym
    assert text.count("triangulate_points(const") >= 2
