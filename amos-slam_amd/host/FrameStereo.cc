// FrameStereo.cc -- host side of ORB_SLAM2::ComputeStereoMatches: sizes the vectors and calls the C ABI; nothing is computed here.
#include "FrameStereo.h"

#include "../../include/amos_frontend.h"

namespace ORB_SLAM2
{

void ComputeStereoMatches(ORBextractor *left, ORBextractor *right, float mbf, float mb, std::vector<float> &mvuRight, std::vector<float> &mvDepth)
{
    const int N = left ? left->LastKeypointCount() : -1;
    mvuRight.assign(N > 0 ? N : 0, -1.0f);  // Frame.cc:1184-1185
    mvDepth.assign(N > 0 ? N : 0, -1.0f);
    if (N <= 0 || !right) return;
    if (amos_frame_stereo_match(left->Handle(), right->Handle(), mbf, mb, mvuRight.data(), mvDepth.data(), N) != AMOS_OK) {
        mvuRight.assign(N, -1.0f);  // the text is in amos_last_error()
        mvDepth.assign(N, -1.0f);
    }
}

}  // namespace ORB_SLAM2
