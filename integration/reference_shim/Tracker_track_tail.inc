// Tracker_track_tail.inc — OPTIONAL edit of a caller: the tail of Tracker::track (track_from_last_frame, optimize_pose,
// match_with_last_key_frame, match_with_map) on the frame's device match table and the resident map, as four calls with no
// host walk over map objects and no list traffic: rs_map_carry_matches, rs_map_refine_pose, rs_map_match_frame twice.
// One download of the table at the end fills the reference's own Frame object, which the mapper reads.
//
// How to apply: in the reference's src/Tracker.cpp, function Tracker::track,
//   KEEP    lines 72-82   (track_features, the Frame, initial_pose_estimate, carry_forward)
//   REPLACE lines 83-86   (the four time_it stages) by
//               #include "Tracker_track_tail.inc"
//   KEEP    line 87       (return frame)
// and add `#include "rs_shim_common.h"` at the top of the file.  Names used from the enclosing scope: frame (the
// std::shared_ptr<Frame> of :77), m_last_frame, m_camera, m_config, inertial_constraint() and MIN_TRACKED_MAP_POINTS
// (:22), and from the caller that owns the resident map (INTEGRATION.md, "The resident map"):
//   rs_map* resident_map                      the map; resident_last_key_frame is last_key_frame's handle in it
//   std::vector<MapPoint*> resident_points    point handle -> object (nullptr once removed)
//   rs_frame* resident_prev, *resident_next   the device frames of m_last_frame and of `frame`: resident_next comes from
//                                             rs_frame_assign_device (which cleared its table), resident_prev is last
//                                             call's resident_next (two device frames swapped frame after frame)
//   const int32_t* resident_kept_index        rs_track_features' d_kept_index (Tracker_track_and_replenish.inc's d_kept)
//   const int32_t* resident_inlier_index, *resident_inlier_count      rs_estimate_pose's; both null when
//                                             initial_pose_estimate returned no inliers (:193-194): nothing is carried
//   int resident_max_n                        the room of those lists
// Requires MapPoint::set_track_consistent to call rs_map_set_track_consistent, and `frame` to hold no map match yet (it
// was constructed at :77).
//
// A removed point still held by m_last_frame's table is a dangling MapPoint* in the reference (undefined behaviour);
// here it is no carry-over candidate and no observation of the refit.
// Results: tests/track_ref.py; the refit is rs_refine_pose_inertial's kernel on the arrays gathered on the device, bit for
// bit (tests/test_gpu_track.py).  motion::is_rotation_plausible stays here (:314).
{
    using namespace rs_shim;
    float K[4], T[16];
    intrinsics(m_camera.get_intrinsic_matrix(), K);
    const int W = m_camera.get_width(), H = m_camera.get_height();
    // :83 track_from_last_frame
    bool done = resident_inlier_count == nullptr ||
                ok(rs_map_carry_matches(context(), resident_map, resident_prev, resident_next, resident_kept_index, resident_inlier_index,
                                        resident_inlier_count, resident_max_n, (int)MIN_TRACKED_MAP_POINTS, nullptr), "rs_map_carry_matches");
    // :84 optimize_pose (:302-320); the :307 gate and refine_pose's own (no point with two observations) are decided on the device
    if (done && m_config.optimize_pose) {
        const optimization::InertialConstraint inertial = inertial_constraint(*frame);
        const auto* prior = std::get_if<optimization::RotationPrior>(&inertial);
        const auto* delta = std::get_if<optimization::InertialDelta>(&inertial);
        int kind = 0;
        double predicted[9] = {}, prev_pose[6] = {}, prev_velocity[3] = {}, prev_bias[6] = {}, velocity[3] = {}, gravity[3] = {};
        rs_imu_factor factor{};
        if (delta != nullptr && delta->enabled()) {                       // src/Optimization.cpp:231-258, as the drop-in's refine_pose packs it
            kind = 2;
            pose_to_row_major(delta->previous->pose(), T);
            rs_pack_pose(T, prev_pose);
            const InertialState& before = delta->previous->inertial();
            const imu::Preintegrated& d = delta->summary;
            factor.duration = d.duration;
            for (int r = 0; r < 3; r++) {
                prev_velocity[r] = before.velocity[r]; prev_bias[r] = before.bias.gyro[r]; prev_bias[3 + r] = before.bias.accel[r];
                velocity[r] = frame->inertial().velocity[r];
                gravity[r] = delta->gravity[r];
                factor.velocity[r] = d.velocity[r]; factor.position[r] = d.position[r];
                factor.bias_gyro[r] = d.bias.gyro[r]; factor.bias_accel[r] = d.bias.accel[r];
                for (int c = 0; c < 3; c++) factor.rotation[3 * r + c] = d.rotation(r, c);
            }
            for (int r = 0; r < 9; r++) {
                for (int c = 0; c < 9; c++) factor.covariance[9 * r + c] = d.covariance(r, c);
                for (int c = 0; c < 6; c++) factor.bias_jacobian[6 * r + c] = d.bias_jacobian(r, c);
            }
            factor.gyro_bias_sigma = delta->noise.gyro_bias; factor.accel_bias_sigma = delta->noise.accel_bias;
        } else if (prior != nullptr && prior->enabled()) {
            kind = 1;
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) predicted[3 * r + c] = prior->predicted(r, c);
        }
        double cam[6];
        pose_to_row_major(frame->pose(), T);
        rs_pack_pose(T, cam);
        rs_ba_summary s{};
        int n_used = 0;
        done = ok(rs_map_refine_pose(context(), resident_map, resident_next, cam, K, (int)MIN_TRACKED_MAP_POINTS, kind, predicted,
                                     prior != nullptr ? prior->sigma_radians : 0.0, prev_pose, prev_velocity, prev_bias, &factor, gravity,
                                     velocity, nullptr, &s, &n_used), "rs_map_refine_pose");
        if (done && n_used > 0) {
            std::printf("refine_pose: iterations %d, cost %.6e -> %.6e, termination %d\n", s.iterations, s.initial_cost, s.final_cost, s.termination);
            if (!s.usable) std::printf("Optimization rejected, unusable or non-improving solution\n");
        }
        if (done && n_used > 0 && s.usable) {
            if (kind == 2) {                                              // src/Optimization.cpp:263-265: kept through a roll-back, as there
                InertialState st;
                st.velocity = Eigen::Vector3d(velocity[0], velocity[1], velocity[2]);
                st.bias.gyro = Eigen::Vector3d(prev_bias[0], prev_bias[1], prev_bias[2]);
                st.bias.accel = Eigen::Vector3d(prev_bias[3], prev_bias[4], prev_bias[5]);
                frame->set_inertial(st);
            }
            rs_unpack_pose(cam, T);
            const Eigen::Matrix4f refined = pose_from_row_major(T);
            if (motion::is_rotation_plausible(m_last_frame->pose(), refined, m_config.seconds_per_frame))     // :314
                frame->set_pose(refined);
            else
                std::cout << "Pose optimization rolled back by temporal motion bound\n";
        }
    }
    // :85 match_with_last_key_frame, :86 match_with_map: one count back per call
    pose_to_row_major(frame->pose(), T);
    int kf_matches = 0, map_matches = 0;
    done = done && ok(rs_map_match_frame(context(), resident_map, resident_next, T, K, W, H, resident_last_key_frame, (int)m_feature_extractor.max_distance(),
                                         &kf_matches), "rs_map_match_frame");
    if (done) std::cout << "Map matches with last frame: " << kf_matches << '\n';
    done = done && ok(rs_map_match_frame(context(), resident_map, resident_next, T, K, W, H, -1, (int)m_feature_extractor.max_distance(),
                                         &map_matches), "rs_map_match_frame");
    if (done) std::cout << "Number of map matches: " << map_matches << '\n';
    // the reference's Frame object follows the device table: keypoint -> point, unique on both sides, so the order of the
    // add_map_match calls does not matter
    std::vector<int32_t> table(frame->features().keypoints.size(), -1);
    int n_matches = 0;
    if (done && ok(rs_frame_matches_download(context(), resident_next, table.data(), &n_matches), "rs_frame_matches_download"))
        for (size_t k = 0; k < table.size(); k++) {
            const int32_t p = table[k];
            if (p >= 0 && (size_t)p < resident_points.size() && resident_points[(size_t)p] != nullptr)
                frame->add_map_match(MapPointMatch{*resident_points[(size_t)p], k});
        }
}
