// Mapper_cull_points.inc — OPTIONAL edit of a caller (SURVEY.md §8(f) rank 3): the projection loop of
// Mapper::cull_points as one rs_point_errors call.
//
// How to apply: in the reference's src/Mapper.cpp, function Mapper::cull_points,
//   KEEP    lines 396-408  (collecting `local`, the points matched by the window's frames)
//   REPLACE lines 410-423  (`points_to_remove` + the per-point reprojection loop and threshold test) by
//               #include "Mapper_cull_points.inc"
//   KEEP    lines 425-431  (log line, diagnostics, Map::remove_point)
// Names used from the enclosing scope: local (std::unordered_set<MapPoint*>), m_camera, MAX_POINT_REPROJECTION_ERROR
// (src/Mapper.cpp:39).  The block leaves behind `points_to_remove` (std::vector<MapPoint*>) as the kept tail reads it,
// and {sum, count} of all per-observation errors in `reprojection_sums`: Slam::reprojection_error()
// (src/Slam.cpp:302-317) is sums[0] / sums[1] over the same observations.
std::vector<MapPoint*> points_to_remove;
double reprojection_sums[2] = {0.0, 0.0};
{
    using namespace rs_shim;
    std::vector<MapPoint*> order(local.begin(), local.end());
    const rs_marshal::PointErrorArrays e = rs_marshal::flatten_point_errors(order, Access{});
    const size_t P = order.size();
    if (P > 0 && !e.obs_pose.empty()) {
        float K[4];
        intrinsics(m_camera.get_intrinsic_matrix(), K);
        Stage stage;
        DevBuf<float> d_pos(e.pos), d_uv(e.uv), d_poses(e.poses), d_mean(P);
        DevBuf<int32_t> d_ptr(e.obs_ptr), d_op(e.obs_pose), d_idx(P), d_cnt(1);
        DevBuf<uint8_t> d_cull(P);
        DevBuf<double> d_sums(2);
        if (ok(rs_point_errors(context(), (int)P, d_pos.p, d_ptr.p, d_op.p, d_uv.p, d_poses.p, e.n_poses, K,
                               MAX_POINT_REPROJECTION_ERROR, d_mean.p, d_cull.p, d_idx.p, d_cnt.p, d_sums.p), "rs_point_errors")) {
            const auto hn = d_cnt.fetch(1);
            const auto hidx = d_idx.fetch(P);
            const auto hs = d_sums.fetch(2);
            stage.sync();
            for (int i = 0; i < hn[0]; i++) points_to_remove.push_back(order[(size_t)hidx[i]]);
            reprojection_sums[0] = hs[0];
            reprojection_sums[1] = hs[1];
        }
    }
}
(void)reprojection_sums;
