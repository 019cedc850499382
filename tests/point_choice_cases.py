"""The hand case of the greedy choice that the motion-model and the relocalisation tests share: one frame, check_orientation on.  A takes
feature 0; B finds it taken and takes its second, feature 1; C finds both taken and the new search gives feature 2; D finds all three
taken and the new search finds nothing.  Built with the hand_frame / hand_query / hand_point helpers of the two restatements."""
import numpy as np

import motion_model_restatement as mr
import reloc_restatement as rr

f32 = np.float32

# (feature aimed at, angle, flipped bits) of A, B, C, D and four fillers.  rot = 36 for A (on angle 0), B (on 96) and the first filler: bin
# 3; 84 for C (on 180) and the second filler: bin 7; 108 for the last two: bin 9.  Three bins stand, so a fourth loses: B's bin from
# feature 0's angle would be 11, C's from feature 0's or 1's 22 or 14.
POINTS = [(0, 36.0, 0), (0, 132.0, 2), (0, 264.0, 3), (0, 300.0, 4), (20, 36.0, 0), (21, 84.0, 0), (22, 108.0, 0), (23, 108.0, 0)]


def frame():
    """mr.hand_frame with features 1 and 2 moved 4 px beside and 4 px below feature 0 (one window with it at a radius above 4) and given
    feature 0's descriptor with bits 100 .. 109 and 120 .. 139 flipped: a record aimed at feature 0 with its first b bits flipped lies at
    b, b + 10 and b + 20 from features 0, 1 and 2.  The three carry the angles 0, 96 and 180, every other feature 0."""
    angles = np.zeros(54, f32)
    angles[1], angles[2] = 96.0, 180.0
    kps, desc = mr.hand_frame(angles)
    kps["x"][1], kps["y"][1] = kps["x"][0] + 4.0, kps["y"][0]
    kps["x"][2], kps["y"][2] = kps["x"][0], kps["y"][0] + 4.0
    for f, bits in ((1, range(100, 110)), (2, range(120, 140))):
        desc[f] = desc[0]
        for b in bits:
            desc[f][b // 8] ^= 1 << (b % 8)
    return kps, desc


def motion_queries(kps, desc):
    """the projected records of the motion-model search, every point with observations"""
    return np.concatenate([mr.hand_query(kps, desc, f, angle=a, has_obs=1, flip_bits=b) for f, a, b in POINTS])


def motion_points(queries):
    """the same records as last-frame points: an identity pose projects (X, Y, 1) onto (512 X + 320, 512 Y + 240)"""
    pts = np.zeros(len(queries), mr.LAST_POINT)
    pts["pos"] = np.stack([(queries["u"] - 320.0) / 512.0, (queries["v"] - 240.0) / 512.0, np.ones(len(queries))], 1)
    pts["angle"], pts["flags"], pts["desc"] = queries["angle"], mr.HAS_OBS, queries["desc"]
    return pts


def reloc_case():
    """the frame on level 4 and the points of the relocalisation search: A, B, C and D aim at feature 0 (level 3, a radius of 3 * 1.728 =
    5.2 px at th = 3: features 1 and 2, 4 px away, share the window), the fillers at features 20 .. 23"""
    kps, desc = frame()
    kps["octave"] = 4
    return kps, desc, [rr.hand_point(kps, desc, f, angle=a, flip_bits=b) for f, a, b in POINTS]
