// stereo_capi.cc -- C entry point that drives ORB_SLAM2::ComputeStereoMatches (amos-slam_amd/host/FrameStereo.h) as the stereo Frame
// constructor would (Frame.cc:165-192): two extractors, two 4-arg operator() calls, then the match.  Test harness: built as
// tests/host_stereo/libamos_host_stereo_test.so, links the product library, never the other way round.
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../include/amos_frontend.h"
#include "../../amos-slam_amd/host/FrameStereo.h"

using namespace ORB_SLAM2;

static thread_local std::string g_error;

extern "C" {

const char *amos_host_stereo_last_error(void) { return g_error.c_str(); }

// pyramid_mode: ORBextractor::PyramidMode for both extractors.  kps_l / desc_l / kps_r / desc_r (cap entries each) receive the two
// extractions, u_right / depth (cap) the match; n[0], n[1] the keypoint counts; rows0 = left.mvImagePyramid[0].rows afterwards.
// break_right != 0: the right extractor gets other parameters (the library must refuse, the vectors must come back all -1).
int amos_host_stereo(const uint8_t *left, const uint8_t *right, int w, int h, int nfeatures, float scale, int nlevels, int ini, int min,
                     int pyramid_mode, int break_right, float mbf, float mb, amos_keypoint *kps_l, uint8_t *desc_l, amos_keypoint *kps_r,
                     uint8_t *desc_r, float *u_right, float *depth, int cap, int32_t *n, int32_t *rows0)
{
    try {
        ORBextractor extL(nfeatures, scale, nlevels, ini, min), extR(break_right ? nfeatures + 100 : nfeatures, scale, nlevels, ini, min);
        extL.SetPyramidMode((ORBextractor::PyramidMode)pyramid_mode);
        extR.SetPyramidMode((ORBextractor::PyramidMode)pyramid_mode);
        cv::Mat imL(h, w, CV_8UC1, (void *)left, (size_t)w), imR(h, w, CV_8UC1, (void *)right, (size_t)w), none, dL, dR;
        std::vector<cv::KeyPoint> kL, kR;
        extL(imL, none, kL, dL);
        extR(imR, none, kR, dR);
        std::vector<float> mvuRight, mvDepth;
        ComputeStereoMatches(&extL, &extR, mbf, mb, mvuRight, mvDepth);
        n[0] = (int)kL.size();
        n[1] = (int)kR.size();
        *rows0 = extL.mvImagePyramid[0].rows;
        if (n[0] > cap || n[1] > cap) return -3;
        if (mvuRight.size() != kL.size() || mvDepth.size() != kL.size()) return -101;
        if (n[0]) std::memcpy(kps_l, kL.data(), sizeof(amos_keypoint) * kL.size());
        if (n[1]) std::memcpy(kps_r, kR.data(), sizeof(amos_keypoint) * kR.size());
        for (int i = 0; i < n[0]; i++) std::memcpy(desc_l + 32 * (size_t)i, dL.ptr(i), 32);
        for (int i = 0; i < n[1]; i++) std::memcpy(desc_r + 32 * (size_t)i, dR.ptr(i), 32);
        if (n[0]) {
            std::memcpy(u_right, mvuRight.data(), sizeof(float) * n[0]);
            std::memcpy(depth, mvDepth.data(), sizeof(float) * n[0]);
        }
        return 0;
    } catch (const std::exception &e) {
        g_error = e.what();
        return -100;
    }
}

}  // extern "C"
