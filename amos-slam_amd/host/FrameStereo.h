// FrameStereo.h -- Frame::ComputeStereoMatches (Frame.cc:1179-1573) for the stereo Frame constructor (Frame.cc:165-192), on the device:
// after the two 4-arg ORBextractor::operator() calls the keypoints, descriptors and pyramid planes of both images are resident on the
// extractors' handles; this function matches them there (amos_frame_stereo_match of include/amos_frontend.h) and copies back the two
// float arrays -- no pyramid plane travels, so both extractors may run with SetPyramidMode(PYRAMID_NEVER).
#ifndef FRAMESTEREO_H
#define FRAMESTEREO_H

#include <vector>

#include "ORBextractor.h"

namespace ORB_SLAM2
{

// mvuRight / mvDepth get one entry per left keypoint, -1 where there is no match.  mbf and mb are Frame's members (mb = mbf / fx, the
// routine's minZ).  Throws nothing: on an error of the library both vectors are all -1 and amos_last_error() holds the text.
void ComputeStereoMatches(ORBextractor *left, ORBextractor *right, float mbf, float mb, std::vector<float> &mvuRight, std::vector<float> &mvDepth);

}  // namespace ORB_SLAM2

#endif
