// LoopDetector_query.inc — OPTIONAL edit of a caller: the two timed stages of LoopDetector::query ("Loop retrieval" and
// "Loop verify") and update_streak on the resident map, with one small read-back per stage and no host pass over the map.
//
// How to apply: in the reference's src/LoopDetector.cpp, function LoopDetector::query,
//   KEEP    lines 484-489  (the two early returns)
//   REPLACE lines 491-509  (rank_candidates(score_candidates(..)), the verify_pnp loop, publish_result, update_streak) by
//               #include "LoopDetector_query.inc"
// and in LoopDetector::Impl replace `bows`, `streak`, `constraints` and `new_loop` (:322-336) by the three members below;
// consume_new_loop() and constraints() (:470-480) forward to m_streak.
// Names used from the enclosing scope: key_frame, key_frames, p_impl->camera, p_impl->last, and three members the edit adds
// to Impl:
//   slam::LoopRetrieval retrieval;      constructed from config.vocabulary_path, seconds_per_frame
//   slam::LoopVerifier verifier;        8192 keypoints, 3 candidates
//   slam::LoopStreak m_streak;
// and from the caller that owns the resident map (INTEGRATION.md, "The resident map"): rs_map* resident_map, in which key
// frame i of `key_frames` is key frame i, and rs_frame* resident_frame, the device-built frame of `key_frame`
// (Session::refresh_descriptors' out_frame) whose rows retrieval.add_key_frame takes from the device.
// Requires every key frame to have been added to the retrieval database when it arrived (one add_key_frame per key
// frame; the reference computes bow_of lazily, :351-353, :366-368).
{
    const size_t from = key_frames.size() - 1;
    const std::vector<slam::LoopCandidate> ranked = p_impl->retrieval.query();                       // "Loop retrieval"
    if (ranked.empty()) {
        p_impl->m_streak.update(from, {}, {}, {});                                                   // :495-499: clears the streak
        p_impl->last = {};
        return;
    }
    std::vector<int32_t> candidate_kfs;
    std::vector<slam::Mat4f> candidate_poses;
    for (const auto& c : ranked) {
        candidate_kfs.push_back((int32_t)c.entry);
        slam::Mat4f pose;
        rs_shim::pose_to_row_major(key_frames[c.entry]->pose(), pose.data());
        candidate_poses.push_back(pose);
    }
    float K[4];
    rs_shim::intrinsics(p_impl->camera.get_intrinsic_matrix(), K);
    const slam::Camera camera(K[0], K[1], K[2], K[3], key_frame.image().cols, key_frame.image().rows);
    const std::vector<slam::LoopVerification> verifications =
        p_impl->verifier.verify(resident_map, (int)from, candidate_kfs, camera);                     // "Loop verify"
    if (verifications.size() != ranked.size()) {
        p_impl->m_streak.update(from, {}, {}, {});
        p_impl->last = {};
        return;
    }
    // publish_result (:287-308): the displayed candidate is best_candidate's
    int32_t display = 0;
    std::vector<rs_loop_result> results;
    for (const auto& v : verifications) results.push_back(v.result);
    rs_loop_best_candidate(results.data(), (int)results.size(), &display);
    LoopQueryResult result;
    for (size_t i = 0; i < ranked.size(); i++)
        result.edges.push_back({key_frame.camera_center(), key_frames[ranked[i].entry]->camera_center(), verifications[i].result.ok != 0});
    const slam::LoopVerification& shown = verifications[(size_t)display];
    result.candidate_index = key_frames[ranked[(size_t)display].entry]->index();
    result.score = ranked[(size_t)display].score;
    result.matches = (size_t)shown.result.inliers;
    result.verified = shown.result.ok != 0;
    result.query = &key_frame;
    result.candidate = key_frames[ranked[(size_t)display].entry].get();
    for (size_t k = 0; k < shown.query_kp.size(); k++) {
        const cv::KeyPoint& q = key_frame.keypoint((size_t)shown.query_kp[k]);
        const cv::KeyPoint& c = result.candidate->keypoint((size_t)shown.candidate_kp[k]);
        result.query_uv.emplace_back(q.pt.x, q.pt.y);
        result.candidate_uv.emplace_back(c.pt.x, c.pt.y);
    }
    p_impl->last = result;
    p_impl->m_streak.update(from, ranked, verifications, candidate_poses);                           // :375-442
}
