// Drop-in replacement of the reference's src/LocalWindow.cpp (keeps src/LocalWindow.h).
// NOT COMPILED IN THIS REPO; see rs_shim_common.h.  Pure pointer-set logic: host only.
#include "LocalWindow.h"

#include "Frame.h"
#include "MapPoint.h"
#include "rs_shim_common.h"

namespace slam::optimization {

std::vector<FrameConfig> build_local_window(const std::vector<std::shared_ptr<KeyFrame>>& key_frames, Frame& new_frame,
                                            size_t window_size, bool fix_oldest)
{
    const int n = (int)key_frames.size();
    const rs_marshal::WindowArrays w = rs_marshal::flatten_local_window(key_frames, new_frame, rs_shim::Access{});
    std::vector<int32_t> of(n + 1);
    std::vector<uint8_t> oo(n + 1);
    int32_t cnt = 0;
    rs_build_local_window(n, w.new_index, (int)window_size, fix_oldest, w.frame_ptr.data(), w.frame_pt.data(), w.pt_ptr.data(),
                          w.pt_obs.data(), of.data(), oo.data(), &cnt);
    std::vector<FrameConfig> out;
    for (int i = 0; i < cnt; i++) out.push_back({oo[i] != 0, of[i] == n ? &new_frame : static_cast<Frame*>(key_frames[of[i]].get())});
    return out;
}

}  // namespace slam::optimization
