// FrameLocalPoints.cc -- host side of ORB_SLAM2::SearchLocalPoints: the calling thread's matcher handle and the call of the C ABI;
// nothing is computed here.
#include "FrameLocalPoints.h"

#include <cstdlib>

namespace ORB_SLAM2
{

namespace
{
struct ThreadMatcher {
    amos_match *h = nullptr;
    ~ThreadMatcher()
    {
        if (h) amos_match_destroy(h);
    }
};
}  // namespace

amos_match *ThreadMatcherHandle()
{
    static thread_local ThreadMatcher tm;
    if (!tm.h) {
        const char *env = std::getenv("AMOS_DEVICE");
        const int device = env ? std::atoi(env) : amos_current_device();
        if (device < 0 || amos_match_create(device, nullptr, &tm.h) != AMOS_OK) return nullptr;
    }
    return tm.h;
}

int SearchLocalPointsArrays(const amos_keypoint *keysUn, const uint8_t *descriptors, const float *uRight, int N, const amos_map_point *points,
                            int nPoints, const amos_local_camera &camera, const uint8_t *occupied, const float *scaleFactors, int nLevels,
                            float minX, float maxX, float minY, float maxY, amos_map_query *query, uint8_t *inView, int32_t *match,
                            amos_local_stats *stats)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    if (amos_match_local_points(h, keysUn, descriptors, uRight, N, points, nPoints, &camera, occupied, scaleFactors, nLevels, minX, maxX, minY,
                                maxY, query, inView, match, stats) != AMOS_OK)
        return -1;
    return stats->n_matches;
}

}  // namespace ORB_SLAM2
