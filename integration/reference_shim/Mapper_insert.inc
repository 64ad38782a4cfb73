// Mapper_insert.inc — OPTIONAL edit of a caller: Mapper::insert on the resident map.  Three blocks, chosen by
// RS_MAPPER_INSERT_PART, replace the three places where the reference walks its own objects per key frame; with
// Mapper_triangulate_tracks.inc (or rs_track_store_triangulate + rs_map_add_track_points, INTEGRATION.md) and
// rs_map_bundle_adjust in between, a key frame costs no host pass over map objects.
//
// How to apply, in the reference's src/Mapper.cpp (add `#include "rs_shim_common.h"` at the top of the file):
//   PART 1  Mapper::insert:         KEEP :155-159, then      #define RS_MAPPER_INSERT_PART 1 / #include "Mapper_insert.inc"
//           (the adoption loop stays for the caller's own objects; the block makes the resident map follow in one call)
//   PART 2  Mapper::bundle_adjust:  REPLACE :379-393 by      #define RS_MAPPER_INSERT_PART 2 / #include "Mapper_insert.inc"
//   PART 3  Mapper::cull_points:    REPLACE :398-431 by      #define RS_MAPPER_INSERT_PART 3 / #include "Mapper_insert.inc"
// Names used from the enclosing scope: key_frame, anchors (:369-375), m_key_frames, m_camera, m_map, diagnostics, BA_WINDOW and
// MAX_POINT_REPROJECTION_ERROR (:21-39), and from the caller that owns the resident map (INTEGRATION.md, "The resident map"):
//   rs_map* resident_map
//   std::vector<MapPoint*> resident_points                        point handle -> object (nullptr once removed)
//   std::unordered_map<const Frame*, int32_t> resident_key_frames key frame -> handle in the map
//   rs_frame* resident_frame                                      the device frame of the frame that becomes the key frame
// Requires Frame::set_pose on a key frame to call rs_map_set_keyframe_pose (the map's pose is "after" in part 2).  The
// MapPoint::set_position calls of part 2 and the Map::remove_point calls of part 3 bring the caller's objects up to date with
// what the map already did: their mutator hooks (INTEGRATION.md) must be off around these blocks — a set_position hook would
// only mark the positions for a re-upload, a remove_point hook is refused by the map (the point is gone) and changes nothing.
// Results: tests/keyframe_ref.py; the arithmetic is rs_reanchor_points' and rs_point_errors', bit for bit
// (tests/test_gpu_keyframe.py).  The compiled and tested counterpart on plain types is slam::insert_key_frame.
#if RS_MAPPER_INSERT_PART == 1
{
    using namespace rs_shim;
    float T[16];
    pose_to_row_major(key_frame->pose(), T);
    int handle = -1, adopted = 0;
    if (ok(rs_map_insert_keyframe(context(), resident_map, resident_frame, T, &handle, &adopted), "rs_map_insert_keyframe"))
        resident_key_frames[key_frame.get()] = handle;
}
#elif RS_MAPPER_INSERT_PART == 2
{
    using namespace rs_shim;
    std::vector<int32_t> kfs;
    std::vector<float> before;
    for (const auto& [frame, pose_before] : anchors) {
        kfs.push_back(resident_key_frames.at(frame));
        append_row_major(pose_before, before);
    }
    std::vector<int32_t> moved(resident_points.size() ? resident_points.size() : 1);
    std::vector<float> xyz(3 * moved.size());
    int n = 0;
    if (ok(rs_map_reanchor(context(), resident_map, kfs.data(), before.data(), (int)kfs.size(), moved.data(), xyz.data(), (int)resident_points.size(), &n),
           "rs_map_reanchor"))
        for (int i = 0; i < n; i++) {
            MapPoint* point = resident_points[(size_t)moved[(size_t)i]];
            if (point != nullptr) point->set_position(Eigen::Vector3f(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]));
        }
}
#elif RS_MAPPER_INSERT_PART == 3
{
    using namespace rs_shim;
    std::vector<int32_t> kfs;
    size_t first = m_key_frames.size() > BA_WINDOW ? m_key_frames.size() - BA_WINDOW : 0;
    for (size_t i = first; i < m_key_frames.size(); i++) kfs.push_back(resident_key_frames.at(m_key_frames[i].get()));
    kfs.push_back(resident_key_frames.at(&key_frame));
    float K[4];
    intrinsics(m_camera.get_intrinsic_matrix(), K);
    std::vector<int32_t> removed(resident_points.size() ? resident_points.size() : 1);
    std::vector<float> xyz(3 * removed.size());
    int n = 0, n_local = 0;
    if (ok(rs_map_cull_points(context(), resident_map, kfs.data(), (int)kfs.size(), K, MAX_POINT_REPROJECTION_ERROR, 1, removed.data(), xyz.data(),
                              (int)resident_points.size(), &n, &n_local), "rs_map_cull_points")) {
        std::cout << "Number of points to remove: " << n << '\n';
        diagnostics.culled.reserve((size_t)n);
        for (int i = 0; i < n; i++) {
            MapPoint*& point = resident_points[(size_t)removed[(size_t)i]];
            diagnostics.culled.push_back(Eigen::Vector3f(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]));
            if (point != nullptr) m_map.remove_point(point);
            point = nullptr;
        }
    }
}
#else
#error "define RS_MAPPER_INSERT_PART as 1, 2 or 3 before including Mapper_insert.inc"
#endif
#undef RS_MAPPER_INSERT_PART
