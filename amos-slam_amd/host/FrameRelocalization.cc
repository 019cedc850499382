// FrameRelocalization.cc -- host side of ORB_SLAM2::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) on the device: the call
// of the C ABI on the calling thread's matcher handle; nothing is computed here.
#include "FrameRelocalization.h"

namespace ORB_SLAM2
{

int SearchRelocalizationArrays(const amos_keypoint *keysUn, const uint8_t *descriptors, int N, const amos_reloc_point *points, int nPoints,
                               const uint8_t *found, const amos_reloc_camera &camera, const float *scaleFactors, int nLevels, float minX, float maxX,
                               float minY, float maxY, amos_kf_query *query, uint8_t *projected, int32_t *match, amos_reloc_stats *stats)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    if (amos_match_reloc(h, keysUn, descriptors, N, points, nPoints, found, &camera, scaleFactors, nLevels, minX, maxX, minY, maxY, query, projected,
                         match, stats) != AMOS_OK)
        return -1;
    return stats->n_matches;
}

}  // namespace ORB_SLAM2
