// FrameRelocalizationPnP.cc -- host side of ORB_SLAM2::DevicePnPsolver: the call of the C ABI on the calling thread's matcher handle;
// nothing is computed here.
#include "FrameRelocalizationPnP.h"

#include "FrameLocalPoints.h"  // ThreadMatcherHandle

namespace ORB_SLAM2
{

int RelocalizationPnPArrays(const amos_keypoint *keysUn, int N, const int32_t *bowMatch, const amos_reloc_point *points, int nPoints,
                            const float *levelSigma2, int nLevels, const amos_reloc_pnp_params &params, void *state, amos_reloc_pnp_result *result,
                            uint8_t *inlier, int32_t *match, uint8_t *found)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    return amos_match_reloc_pnp(h, keysUn, N, bowMatch, points, nPoints, levelSigma2, nLevels, &params, state, result, inlier, match, found) == AMOS_OK ? 0 : -1;
}

size_t RelocalizationPnPStateBytes(int N) { return amos_reloc_pnp_state_bytes(N > 1 ? N : 1); }

}  // namespace ORB_SLAM2
