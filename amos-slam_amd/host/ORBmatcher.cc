// ORBmatcher.cc -- see ORBmatcher.h.  Line references are to the reference's src/ORBmatcher.cc and
// src/Frame.cc.
#include "ORBmatcher.h"

#include <climits>
#include <cmath>
#include <mutex>
#include <stdexcept>
#include <string>

using namespace std;

namespace ORB_SLAM2
{

const int AMOS_VIEW_MATCHER::TH_HIGH = 100;
const int AMOS_VIEW_MATCHER::TH_LOW = 50;
const int AMOS_VIEW_MATCHER::HISTO_LENGTH = 30;

static void Check(int rc, const char *what)
{
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + amos_last_error());
}

// ---------------------------------------------------------------------------------------------
FeatureGrid::FeatureGrid(const amos_frame_view &frame) : mFrame(frame)
{
    mfGridElementWidthInv = static_cast<float>(AMOS_FRAME_GRID_COLS) / static_cast<float>(frame.max_x - frame.min_x);   // Frame.cc:302
    mfGridElementHeightInv = static_cast<float>(AMOS_FRAME_GRID_ROWS) / static_cast<float>(frame.max_y - frame.min_y);
    for (int i = 0; i < frame.n; i++) {  // AssignFeaturesToGrid, Frame.cc:431-461
        int nGridPosX, nGridPosY;
        if (PosInGrid(frame.keys_un[i], nGridPosX, nGridPosY)) mGrid[nGridPosX][nGridPosY].push_back(i);
    }
}

bool FeatureGrid::PosInGrid(const amos_keypoint &kp, int &posX, int &posY) const
{
    posX = round((kp.x - mFrame.min_x) * mfGridElementWidthInv);  // Frame.cc:1019-1020
    posY = round((kp.y - mFrame.min_y) * mfGridElementHeightInv);
    if (posX < 0 || posX >= AMOS_FRAME_GRID_COLS || posY < 0 || posY >= AMOS_FRAME_GRID_ROWS) return false;
    return true;
}

// Frame.cc:894-1003, appending to vIndices
void FeatureGrid::AppendFeaturesInArea(vector<int> &vIndices, const float &x, const float &y, const float &r, const int minLevel,
                                       const int maxLevel) const
{
    const int nMinCellX = max(0, (int)floor((x - mFrame.min_x - r) * mfGridElementWidthInv));
    if (nMinCellX >= AMOS_FRAME_GRID_COLS) return;
    const int nMaxCellX = min((int)AMOS_FRAME_GRID_COLS - 1, (int)ceil((x - mFrame.min_x + r) * mfGridElementWidthInv));
    if (nMaxCellX < 0) return;
    const int nMinCellY = max(0, (int)floor((y - mFrame.min_y - r) * mfGridElementHeightInv));
    if (nMinCellY >= AMOS_FRAME_GRID_ROWS) return;
    const int nMaxCellY = min((int)AMOS_FRAME_GRID_ROWS - 1, (int)ceil((y - mFrame.min_y + r) * mfGridElementHeightInv));
    if (nMaxCellY < 0) return;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
        for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
            const vector<size_t> &vCell = mGrid[ix][iy];
            if (vCell.empty()) continue;
            for (size_t j = 0, jend = vCell.size(); j < jend; j++) {
                const amos_keypoint &kpUn = mFrame.keys_un[vCell[j]];
                if (bCheckLevels) {
                    if (kpUn.octave < minLevel) continue;
                    if (maxLevel >= 0)
                        if (kpUn.octave > maxLevel) continue;
                }
                const float distx = kpUn.x - x;
                const float disty = kpUn.y - y;
                if (fabs(distx) < r && fabs(disty) < r) vIndices.push_back((int)vCell[j]);
            }
        }
    }
}

vector<size_t> FeatureGrid::GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel, const int maxLevel) const
{
    vector<int> vIndices;
    AppendFeaturesInArea(vIndices, x, y, r, minLevel, maxLevel);
    return vector<size_t>(vIndices.begin(), vIndices.end());
}

// ---------------------------------------------------------------------------------------------
// The reference constructs a matcher ON THE STACK at every call site (Tracking.cc:1492,1744,1910,2378,2609,2663, LocalMapping.cc:324,669,
// LoopClosing.cc:346,813): several per frame, from three threads.  Its constructor stores two numbers (ORBmatcher.cc:49-51), so must this
// one: the device handle (HIP stream + scratch buffers that grow to the largest search seen) is borrowed from a process-wide pool on the
// FIRST search of the object and handed back by the destructor -- no HIP call in either, no hipMalloc / hipFree / stream churn per frame.
// A handle serves one matcher object at a time (it is re-entrant across objects, not within one); the pool is per device and lives as long
// as the process (like the extractors Tracking never frees, Tracking.cc:172-185): destroying HIP objects from a static destructor after the
// runtime has shut down is not defined.
namespace
{
struct MatchPool {
    std::mutex mutex;
    std::vector<std::vector<amos_match *> > idle;  // [device]
    int created = 0;
};
MatchPool &Pool()
{
    static MatchPool *pool = new MatchPool();  // never deleted, see above
    return *pool;
}
}  // namespace

extern int AmosPickDevice();  // ORBextractor.cc: AMOS_DEVICE, else the calling thread's current HIP device

amos_match *AMOS_VIEW_MATCHER::Handle()
{
    if (mpMatch) return mpMatch;
    mnDevice = AmosPickDevice();
    MatchPool &pool = Pool();
    {
        std::lock_guard<std::mutex> lock(pool.mutex);
        if ((int)pool.idle.size() > mnDevice && !pool.idle[mnDevice].empty()) {
            mpMatch = pool.idle[mnDevice].back();
            pool.idle[mnDevice].pop_back();
            return mpMatch;
        }
        pool.created++;
    }
    Check(amos_match_create(mnDevice, nullptr, &mpMatch), "amos_match_create");
    return mpMatch;
}

int AMOS_VIEW_MATCHER::PoolHandlesCreated()
{
    MatchPool &pool = Pool();
    std::lock_guard<std::mutex> lock(pool.mutex);
    return pool.created;
}

AMOS_VIEW_MATCHER::AMOS_VIEW_MATCHER(float nnratio, bool checkOri) : mfNNratio(nnratio), mbCheckOrientation(checkOri), mpMatch(nullptr), mnDevice(-1)
{
}

AMOS_VIEW_MATCHER::~AMOS_VIEW_MATCHER()
{
    if (!mpMatch) return;
    MatchPool &pool = Pool();
    std::lock_guard<std::mutex> lock(pool.mutex);
    if ((int)pool.idle.size() <= mnDevice) pool.idle.resize(mnDevice + 1);
    pool.idle[mnDevice].push_back(mpMatch);  // every call on a handle is synchronous: nothing of this object is in flight
}

// ORBmatcher.cc:1913-1933: one pair.  Callers use it inside host loops (MapPoint::ComputeDistinctiveDescriptors,
// Frame / KeyFrame bookkeeping), so a single pair is eight host popcounts, not a kernel launch; sets of descriptors
// go through DescriptorDistances / the Search* functions (GPU).
int AMOS_VIEW_MATCHER::DescriptorDistance(const cv::Mat &a, const cv::Mat &b)
{
    const unsigned char *pa = a.ptr(), *pb = b.ptr();
    int dist = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x, y;
        memcpy(&x, pa + 4 * i, 4);
        memcpy(&y, pb + 4 * i, 4);
        dist += __builtin_popcount(x ^ y);
    }
    return dist;
}

void AMOS_VIEW_MATCHER::DescriptorDistances(const uint8_t *q, int nq, const uint8_t *t, int nt, std::vector<uint16_t> &out)
{
    out.resize((size_t)nq * nt);
    Check(amos_match_distances(Handle(), q, nq, t, nt, out.data()), "amos_match_distances");
}

// ---------------------------------------------------------------------------------------------
// The pieces every search is built from: candidate lists (with the one GPU call and the scans over its result) and the
// rotation histogram.  Each search below is then: candidates, scan, its own accept rule, prune.

// The candidate lists of all queries of a search, in CSR form: query i's candidates are idx[off[i] .. off[i + 1]), dist[] their
// distances.  A list is filled by Open(), then pushing onto idx (Open() and Distances() close the list before).
struct AMOS_VIEW_MATCHER::CandidateLists {
    vector<int> off, idx;
    vector<uint8_t> qdesc;  // the queries' descriptors, 32 bytes each
    vector<uint16_t> dist;

    explicit CandidateLists(int nq = 0)
    {
        off.reserve(nq + 1);
        off.push_back(0);
        qdesc.reserve((size_t)nq * 32);
    }
    // next query; desc = nullptr when the caller hands Distances() a descriptor block of its own
    void Open(const uint8_t *desc = nullptr)
    {
        off.back() = (int)idx.size();
        off.push_back(off.back());
        if (desc) qdesc.insert(qdesc.end(), desc, desc + 32);
    }
    bool Empty(int i) const { return off[i] == off[i + 1]; }

    // all candidate distances in one GPU call
    void Distances(AMOS_VIEW_MATCHER &m, const uint8_t *train, int nt, const uint8_t *queries = nullptr)
    {
        off.back() = (int)idx.size();
        dist.resize(idx.size());
        if (idx.empty()) return;
        Check(amos_match_list_distances(m.Handle(), queries ? queries : qdesc.data(), (int)off.size() - 1, train, nt, off.data(), idx.data(),
                                        dist.data()),
              "amos_match_list_distances");
    }

    // Best candidate of query i among those skip(candidate, distance) lets through: the FIRST of the smallest distance below
    // the value bestDist comes in with, or -1.
    template <typename Skip>
    int Best(int i, int &bestDist, Skip skip) const
    {
        int bestIdx = -1;
        for (int k = off[i]; k < off[i + 1]; k++) {
            const int d = dist[k];
            if (skip(idx[k], d)) continue;
            if (d < bestDist) {
                bestDist = d;
                bestIdx = idx[k];
            }
        }
        return bestIdx;
    }
    int Best(int i, int &bestDist) const
    {
        return Best(i, bestDist, [](int, int) { return false; });
    }
    // ... and the second best distance (with its candidate, when asked for)
    template <typename Skip>
    int Best2(int i, int &bestDist, int &bestDist2, Skip skip, int *pBestIdx2 = nullptr) const
    {
        int bestIdx = -1, bestIdx2 = -1;
        for (int k = off[i]; k < off[i + 1]; k++) {
            const int d = dist[k];
            if (skip(idx[k], d)) continue;
            if (d < bestDist) {
                bestDist2 = bestDist;
                bestDist = d;
                bestIdx2 = bestIdx;
                bestIdx = idx[k];
            } else if (d < bestDist2) {
                bestDist2 = d;
                bestIdx2 = idx[k];
            }
        }
        if (pBestIdx2) *pBestIdx2 = bestIdx2;
        return bestIdx;
    }

    // Node-by-node search between two feature vectors (ORBmatcher.cc:248-339, :673-760, :835-935): for every feature of side A
    // that take1 accepts (q1 lists them), the features of side B in the same node, in the FeatureVector's order.  The two-iterator
    // merge over the ascending node ids is the reference's (lower_bound on a std::map = first node id >= the other side's).
    template <typename Take1>
    void OpenSharedNodes(const amos_bow_view &A, const amos_bow_view &B, Take1 take1, vector<int> &q1)
    {
        int a = 0, b = 0;
        while (a < A.n_nodes && b < B.n_nodes) {
            if (A.node_ids[a] == B.node_ids[b]) {
                for (int k = A.node_off[a]; k < A.node_off[a + 1]; k++) {
                    const int idx1 = A.node_idx[k];
                    if (!take1(idx1)) continue;
                    q1.push_back(idx1);
                    Open(A.descriptors + (size_t)idx1 * 32);
                    idx.insert(idx.end(), B.node_idx + B.node_off[b], B.node_idx + B.node_off[b + 1]);
                }
                a++;
                b++;
            } else if (A.node_ids[a] < B.node_ids[b]) {
                while (a < A.n_nodes && A.node_ids[a] < B.node_ids[b]) a++;
            } else {
                while (b < B.n_nodes && B.node_ids[b] < A.node_ids[a]) b++;
            }
        }
    }
};

namespace
{
// The orientation check the six oriented searches end with (e.g. ORBmatcher.cc:1693-1725): every accepted match votes with its
// angle difference, and the matches outside the three fullest bins are taken back.
struct RotationHistogram {
    vector<int> bins[AMOS_VIEW_MATCHER::HISTO_LENGTH];

    RotationHistogram()
    {
        for (vector<int> &bin : bins) bin.reserve(500);
    }
    // slot: the entry of the search's match table that Prune() clears if this vote loses
    void Add(float angleQuery, float angleTrain, int slot)
    {
        const float factor = AMOS_VIEW_MATCHER::HISTO_LENGTH / 360.0f;
        float rot = angleQuery - angleTrain;
        if (rot < 0.0) rot += 360.0f;
        int bin = round(rot * factor);
        if (bin == AMOS_VIEW_MATCHER::HISTO_LENGTH) bin = 0;
        bins[bin].push_back(slot);
    }
    // Returns the number of matches to subtract: one per VOTE, not per slot -- a slot that was overwritten during the search and
    // voted twice counts twice, which is the reference's accounting.  onlyIfSet: leave out votes whose slot is clear already.
    int Prune(vector<int> &table, int freeValue, bool onlyIfSet = false)
    {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        AMOS_VIEW_MATCHER::ComputeThreeMaxima(bins, AMOS_VIEW_MATCHER::HISTO_LENGTH, ind1, ind2, ind3);
        int removed = 0;
        for (int i = 0; i < AMOS_VIEW_MATCHER::HISTO_LENGTH; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (size_t j = 0, jend = bins[i].size(); j < jend; j++) {
                const int slot = bins[i][j];
                if (onlyIfSet && table[slot] < 0) continue;
                table[slot] = freeValue;
                removed++;
            }
        }
        return removed;
    }
};
}  // namespace

float AMOS_VIEW_MATCHER::RadiusByViewingCos(const float &viewCos)
{
    if (viewCos > 0.998)
        return 2.5;
    else
        return 4.0;
}

// ORBmatcher.cc:1569-1728
int AMOS_VIEW_MATCHER::SearchByProjection(const FeatureGrid &CurrentFrame, const vector<amos_proj_query> &vLastPoints, vector<int> &vnCurMatch,
                                   const vector<float> &mvScaleFactors, float mbf, const float th, const bool bForward, const bool bBackward)
{
    const amos_frame_view &F = CurrentFrame.Frame();
    const int nq = (int)vLastPoints.size();
    CandidateLists c(nq);  // in GetFeaturesInArea order (:1627-1637)
    vector<float> radius(nq);
    for (int i = 0; i < nq; i++) {
        const amos_proj_query &p = vLastPoints[i];
        const int nLastOctave = p.octave;
        radius[i] = th * mvScaleFactors[nLastOctave];
        c.Open(p.desc);
        if (bForward)
            CurrentFrame.AppendFeaturesInArea(c.idx, p.u, p.v, radius[i], nLastOctave);
        else if (bBackward)
            CurrentFrame.AppendFeaturesInArea(c.idx, p.u, p.v, radius[i], 0, nLastOctave);
        else
            CurrentFrame.AppendFeaturesInArea(c.idx, p.u, p.v, radius[i], nLastOctave - 1, nLastOctave + 1);
    }
    c.Distances(*this, F.descriptors, F.n);
    int nmatches = 0;
    RotationHistogram rotHist;
    for (int i = 0; i < nq; i++) {
        if (c.Empty(i)) continue;
        const amos_proj_query &p = vLastPoints[i];
        int bestDist = 256;
        const int bestIdx2 = c.Best(i, bestDist, [&](int i2, int) {
            if (vnCurMatch[i2] >= 0)
                if (vLastPoints[vnCurMatch[i2]].has_obs) return true;  // :1658-1660
            if (F.u_right && F.u_right[i2] > 0) {                       // :1662-1669
                const float ur = p.u - mbf * p.invz;
                const float er = fabs(ur - F.u_right[i2]);
                if (er > radius[i]) return true;
            }
            return false;
        });
        if (bestDist <= TH_HIGH) {
            vnCurMatch[bestIdx2] = i;  // may overwrite an occupant without observations, whose vote stays in the histogram
            nmatches++;
            if (mbCheckOrientation) rotHist.Add(p.angle, F.keys_un[bestIdx2].angle, bestIdx2);
        }
    }
    if (mbCheckOrientation) nmatches -= rotHist.Prune(vnCurMatch, -1);
    return nmatches;
}

// ORBmatcher.cc:70-175
int AMOS_VIEW_MATCHER::SearchByProjection(const FeatureGrid &Fg, const vector<amos_map_query> &vpMapPoints, vector<int> &vnCurMatch,
                                   vector<bool> &vbCurHasObs, const vector<float> &mvScaleFactors, const float th)
{
    const amos_frame_view &F = Fg.Frame();
    const int nq = (int)vpMapPoints.size();
    const bool bFactor = th != 1.0;
    CandidateLists c(nq);
    vector<float> rr(nq);
    for (int iMP = 0; iMP < nq; iMP++) {
        const amos_map_query &mp = vpMapPoints[iMP];
        const int nPredictedLevel = mp.level;
        float r = RadiusByViewingCos(mp.view_cos);
        if (bFactor) r *= th;
        rr[iMP] = r;
        c.Open(mp.desc);
        Fg.AppendFeaturesInArea(c.idx, mp.proj_x, mp.proj_y, r * mvScaleFactors[nPredictedLevel], nPredictedLevel - 1, nPredictedLevel);
    }
    c.Distances(*this, F.descriptors, F.n);
    int nmatches = 0;
    for (int iMP = 0; iMP < nq; iMP++) {
        if (c.Empty(iMP)) continue;
        const amos_map_query &mp = vpMapPoints[iMP];
        const int nPredictedLevel = mp.level;
        const float r = rr[iMP];
        int bestDist = 256, bestDist2 = 256, bestIdx2 = -1;
        const int bestIdx = c.Best2(iMP, bestDist, bestDist2,
                                    [&](int i, int) {
                                        if (vbCurHasObs[i]) return true;  // :121-123
                                        if (F.u_right && F.u_right[i] > 0) {
                                            const float er = fabs(mp.proj_xr - F.u_right[i]);
                                            if (er > r * mvScaleFactors[nPredictedLevel]) return true;
                                        }
                                        return false;
                                    },
                                    &bestIdx2);
        if (bestDist <= TH_HIGH) {
            const int bestLevel = F.keys_un[bestIdx].octave, bestLevel2 = bestIdx2 >= 0 ? F.keys_un[bestIdx2].octave : -1;
            if (bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2) continue;  // :163-167
            vnCurMatch[bestIdx] = iMP;
            vbCurHasObs[bestIdx] = mp.has_obs != 0;
            nmatches++;
        }
    }
    return nmatches;
}

// ORBmatcher.cc:1731-1863 (relocalisation): window nPredictedLevel-1 .. +1, ANY occupied feature is skipped,
// best only, accepted at bestDist <= ORBdist.
int AMOS_VIEW_MATCHER::SearchByProjection(const FeatureGrid &CurrentFrame, const vector<amos_kf_query> &vKFPoints, vector<int> &vnCurMatch,
                                   const vector<float> &mvScaleFactors, const float th, const int ORBdist)
{
    const amos_frame_view &F = CurrentFrame.Frame();
    const int nq = (int)vKFPoints.size();
    CandidateLists c(nq);
    for (int i = 0; i < nq; i++) {
        const amos_kf_query &p = vKFPoints[i];
        const int nPredictedLevel = p.level;
        const float radius = th * mvScaleFactors[nPredictedLevel];
        c.Open(p.desc);
        CurrentFrame.AppendFeaturesInArea(c.idx, p.u, p.v, radius, nPredictedLevel - 1, nPredictedLevel + 1);
    }
    c.Distances(*this, F.descriptors, F.n);
    int nmatches = 0;
    RotationHistogram rotHist;
    for (int i = 0; i < nq; i++) {
        if (c.Empty(i)) continue;  // :1802-1803
        int bestDist = 256;
        const int bestIdx2 = c.Best(i, bestDist, [&](int i2, int) { return vnCurMatch[i2] != AMOS_MATCH_FREE; });  // :1816-1817
        if (bestDist <= ORBdist) {
            vnCurMatch[bestIdx2] = i;
            nmatches++;
            if (mbCheckOrientation) rotHist.Add(vKFPoints[i].angle, F.keys_un[bestIdx2].angle, bestIdx2);
        }
    }
    if (mbCheckOrientation) nmatches -= rotHist.Prune(vnCurMatch, AMOS_MATCH_FREE);
    return nmatches;
}

// ORBmatcher.cc:230-382.  Candidates of a keyframe feature = the frame's features in the same vocabulary node.
int AMOS_VIEW_MATCHER::SearchByBoW(const amos_bow_view &KF, const amos_bow_view &F, vector<int> &vnMatchesF)
{
    vnMatchesF.assign(F.n, -1);
    vector<int> qKF;
    CandidateLists c;
    c.OpenSharedNodes(KF, F, [&](int iKF) { return !KF.has_point || KF.has_point[iKF]; }, qKF);  // pMP && !pMP->isBad()
    c.Distances(*this, F.descriptors, F.n);
    int nmatches = 0;
    RotationHistogram rotHist;
    for (int i = 0, nq = (int)qKF.size(); i < nq; i++) {
        const int realIdxKF = qKF[i];
        int bestDist1 = 256, bestDist2 = 256;
        const int bestIdxF = c.Best2(i, bestDist1, bestDist2, [&](int realIdxF, int) { return vnMatchesF[realIdxF] >= 0; });  // :288-289
        if (bestDist1 <= TH_LOW) {
            if (static_cast<float>(bestDist1) < mfNNratio * static_cast<float>(bestDist2)) {
                vnMatchesF[bestIdxF] = realIdxKF;
                if (mbCheckOrientation) rotHist.Add(KF.keys[realIdxKF].angle, F.keys[bestIdxF].angle, bestIdxF);
                nmatches++;
            }
        }
    }
    if (mbCheckOrientation) nmatches -= rotHist.Prune(vnMatchesF, -1);
    return nmatches;
}

// ORBmatcher.cc:656-808
int AMOS_VIEW_MATCHER::SearchByBoW(const amos_bow_view &KF1, const amos_bow_view &KF2, vector<int> &vnMatches12, const bool bBothKeyFrames)
{
    if (!bBothKeyFrames) return SearchByBoW(KF1, KF2, vnMatches12);
    vnMatches12.assign(KF1.n, -1);
    vector<bool> vbMatched2(KF2.n, false);
    vector<int> q1;
    CandidateLists c;
    c.OpenSharedNodes(KF1, KF2, [&](int i1) { return !KF1.has_point || KF1.has_point[i1]; }, q1);
    c.Distances(*this, KF2.descriptors, KF2.n);
    RotationHistogram rotHist;
    int nmatches = 0;
    for (int i = 0, nq = (int)q1.size(); i < nq; i++) {
        const int idx1 = q1[i];
        int bestDist1 = 256, bestDist2 = 256;
        const int bestIdx2 = c.Best2(i, bestDist1, bestDist2,
                                     [&](int idx2, int) { return vbMatched2[idx2] || (KF2.has_point && !KF2.has_point[idx2]); });  // :704-708
        if (bestDist1 < TH_LOW) {  // strict here, <= in SearchByBoW(KF, F)
            if (static_cast<float>(bestDist1) < mfNNratio * static_cast<float>(bestDist2)) {
                vnMatches12[idx1] = bestIdx2;
                vbMatched2[bestIdx2] = true;
                if (mbCheckOrientation) rotHist.Add(KF1.keys[idx1].angle, KF2.keys[bestIdx2].angle, idx1);
                nmatches++;
            }
        }
    }
    if (mbCheckOrientation) nmatches -= rotHist.Prune(vnMatches12, -1);
    return nmatches;
}

// ORBmatcher.cc:188-215 (no fused multiply-add: every product and sum rounds to float as written)
bool AMOS_VIEW_MATCHER::CheckDistEpipolarLine(const amos_keypoint &kp1, const amos_keypoint &kp2, const float F12[9], float sigma2_kp2)
{
    const float a = kp1.x * F12[0] + kp1.y * F12[3] + F12[6];
    const float b = kp1.x * F12[1] + kp1.y * F12[4] + F12[7];
    const float c = kp1.x * F12[2] + kp1.y * F12[5] + F12[8];
    const float num = a * kp2.x + b * kp2.y + c;
    const float den = a * a + b * b;
    if (den == 0) return false;
    const float dsqr = num * num / den;
    return dsqr < 3.84 * sigma2_kp2;
}

// ORBmatcher.cc:810-1018
int AMOS_VIEW_MATCHER::SearchForTriangulation(const amos_bow_view &KF1, const amos_bow_view &KF2, const float F12[9], float ex, float ey,
                                       const vector<float> &mvScaleFactors2, const vector<float> &mvLevelSigma2_2,
                                       vector<pair<size_t, size_t> > &vMatchedPairs, const bool bOnlyStereo)
{
    auto stereo = [](const amos_bow_view &v, int i) { return v.u_right ? v.u_right[i] >= 0 : false; };
    vector<int> q1;
    CandidateLists c;
    c.OpenSharedNodes(KF1, KF2,
                      [&](int i1) {
                          if (KF1.has_point && KF1.has_point[i1]) return false;  // pMP1 exists: nothing to triangulate (:846-849)
                          if (bOnlyStereo && !stereo(KF1, i1)) return false;
                          return true;
                      },
                      q1);
    c.Distances(*this, KF2.descriptors, KF2.n);
    int nmatches = 0;
    vector<bool> vbMatched2(KF2.n, false);
    vector<int> vMatches12(KF1.n, -1);
    RotationHistogram rotHist;
    for (int i = 0, nq = (int)q1.size(); i < nq; i++) {
        const int idx1 = q1[i];
        const bool bStereo1 = stereo(KF1, idx1);
        const amos_keypoint &kp1 = KF1.keys[idx1];
        // Not an argmin: a later candidate of EQUAL distance that passes the geometric tests replaces an earlier one (d > bestDist skips).
        int bestDist = TH_LOW;
        int bestIdx2 = -1;
        for (int k = c.off[i]; k < c.off[i + 1]; k++) {
            const int idx2 = c.idx[k];
            if (vbMatched2[idx2] || (KF2.has_point && KF2.has_point[idx2])) continue;  // :866-869
            const bool bStereo2 = stereo(KF2, idx2);
            if (bOnlyStereo)
                if (!bStereo2) continue;
            const int d = c.dist[k];
            if (d > TH_LOW || d > bestDist) continue;
            const amos_keypoint &kp2 = KF2.keys[idx2];
            if (!bStereo1 && !bStereo2) {
                const float distex = ex - kp2.x;
                const float distey = ey - kp2.y;
                if (distex * distex + distey * distey < 100 * mvScaleFactors2[kp2.octave]) continue;
            }
            if (CheckDistEpipolarLine(kp1, kp2, F12, mvLevelSigma2_2[kp2.octave])) {
                bestIdx2 = idx2;
                bestDist = d;
            }
        }
        if (bestIdx2 >= 0) {
            vMatches12[idx1] = bestIdx2;
            vbMatched2[bestIdx2] = true;
            nmatches++;
            if (mbCheckOrientation) rotHist.Add(kp1.angle, KF2.keys[bestIdx2].angle, idx1);
        }
    }
    if (mbCheckOrientation) nmatches -= rotHist.Prune(vMatches12, -1);
    vMatchedPairs.clear();
    vMatchedPairs.reserve(nmatches);
    for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
        if (vMatches12[i] < 0) continue;
        vMatchedPairs.push_back(make_pair(i, (size_t)vMatches12[i]));
    }
    return nmatches;
}

// The candidates shared by Fuse (:1086-1127, :1252-1272), SearchByProjection(pKF, Scw, ...) (:466-494) and SearchBySim3
// (:1396-1420, :1476-1500): KeyFrame::GetFeaturesInArea(u, v, th * scale) has no level filter; the level gate
// kpLevel < nPredictedLevel-1 || kpLevel > nPredictedLevel  and, when mvInvLevelSigma2 is given, Fuse's chi2 gate on the
// reprojection error follow per candidate.
void AMOS_VIEW_MATCHER::WindowCandidates(const FeatureGrid &KF, const vector<amos_window_query> &q, const vector<float> &mvScaleFactors, const float th,
                                  const vector<float> *mvInvLevelSigma2, CandidateLists &c)
{
    const amos_frame_view &F = KF.Frame();
    for (size_t i = 0; i < q.size(); i++) {
        const amos_window_query &p = q[i];
        const int nPredictedLevel = p.level;
        const float radius = th * mvScaleFactors[nPredictedLevel];
        c.Open(p.desc);
        const size_t first = c.idx.size();
        KF.AppendFeaturesInArea(c.idx, p.u, p.v, radius);
        size_t kept = first;  // the gates below compact the window's features in place
        for (size_t k = first; k < c.idx.size(); k++) {
            const int i2 = c.idx[k];
            const amos_keypoint &kp = F.keys_un[i2];
            const int kpLevel = kp.octave;
            if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
            if (mvInvLevelSigma2) {
                if (F.u_right && F.u_right[i2] >= 0) {  // :1102-1116
                    const float ex = p.u - kp.x;
                    const float ey = p.v - kp.y;
                    const float er = p.ur - F.u_right[i2];
                    const float e2 = ex * ex + ey * ey + er * er;
                    if (e2 * (*mvInvLevelSigma2)[kpLevel] > 7.8) continue;
                } else {
                    const float ex = p.u - kp.x;
                    const float ey = p.v - kp.y;
                    const float e2 = ex * ex + ey * ey;
                    if (e2 * (*mvInvLevelSigma2)[kpLevel] > 5.99) continue;
                }
            }
            c.idx[kept++] = i2;
        }
        c.idx.resize(kept);
    }
    c.Distances(*this, F.descriptors, F.n);
}

// vnBestIdx[i] = the nearest window candidate of query i if its distance is <= maxDist, else -1; returns how many were found
int AMOS_VIEW_MATCHER::BestInWindow(const FeatureGrid &KF, const vector<amos_window_query> &q, const vector<float> &mvScaleFactors, const float th,
                             const vector<float> *mvInvLevelSigma2, const int maxDist, vector<int> &vnBestIdx)
{
    CandidateLists c((int)q.size());
    WindowCandidates(KF, q, mvScaleFactors, th, mvInvLevelSigma2, c);
    int nFound = 0;
    vnBestIdx.assign(q.size(), -1);
    for (int i = 0; i < (int)q.size(); i++) {
        int bestDist = 256;
        const int bestIdx = c.Best(i, bestDist);
        if (bestDist <= maxDist) {
            vnBestIdx[i] = bestIdx;
            nFound++;
        }
    }
    return nFound;
}

// ORBmatcher.cc:1020-1177
int AMOS_VIEW_MATCHER::Fuse(const FeatureGrid &KF, const vector<amos_window_query> &vpMapPoints, const vector<float> &mvScaleFactors,
                     const vector<float> &mvInvLevelSigma2, const float th, vector<int> &vnBestIdx)
{
    return BestInWindow(KF, vpMapPoints, mvScaleFactors, th, &mvInvLevelSigma2, TH_LOW, vnBestIdx);
}

// ORBmatcher.cc:1179-1312
int AMOS_VIEW_MATCHER::Fuse(const FeatureGrid &KF, const vector<amos_window_query> &vpPoints, const vector<float> &mvScaleFactors, const float th,
                     vector<int> &vnBestIdx)
{
    return BestInWindow(KF, vpPoints, mvScaleFactors, th, nullptr, TH_LOW, vnBestIdx);
}

// ORBmatcher.cc:388-512
int AMOS_VIEW_MATCHER::SearchByProjection(const FeatureGrid &KF, const vector<amos_window_query> &vpPoints, vector<int> &vnMatched,
                                   const vector<float> &mvScaleFactors, const int th)
{
    CandidateLists c((int)vpPoints.size());
    WindowCandidates(KF, vpPoints, mvScaleFactors, (float)th, nullptr, c);
    int nmatches = 0;
    for (int i = 0; i < (int)vpPoints.size(); i++) {
        int bestDist = 256;
        const int bestIdx = c.Best(i, bestDist, [&](int idx, int) { return vnMatched[idx] != AMOS_MATCH_FREE; });  // :470-471
        if (bestDist <= TH_LOW) {
            vnMatched[bestIdx] = i;
            nmatches++;
        }
    }
    return nmatches;
}

// ORBmatcher.cc:1314-1565
int AMOS_VIEW_MATCHER::SearchBySim3(const FeatureGrid &KF1, const FeatureGrid &KF2, const vector<amos_window_query> &v1in2,
                             const vector<amos_window_query> &v2in1, const vector<float> &mvScaleFactors1, const vector<float> &mvScaleFactors2,
                             vector<int> &vnMatches12, const float th)
{
    const int N1 = KF1.Frame().n, N2 = KF2.Frame().n;
    vector<int> vnMatch1(N1, -1), vnMatch2(N2, -1), vnBestIdx;
    BestInWindow(KF2, v1in2, mvScaleFactors2, th, nullptr, TH_HIGH, vnBestIdx);  // KF1's points searched in KF2
    for (size_t i = 0; i < v1in2.size(); i++)
        if (vnBestIdx[i] >= 0) vnMatch1[v1in2[i].src] = vnBestIdx[i];
    BestInWindow(KF1, v2in1, mvScaleFactors1, th, nullptr, TH_HIGH, vnBestIdx);  // KF2's points searched in KF1
    for (size_t i = 0; i < v2in1.size(); i++)
        if (vnBestIdx[i] >= 0) vnMatch2[v2in1[i].src] = vnBestIdx[i];
    vnMatches12.assign(N1, -1);
    int nFound = 0;
    for (int i1 = 0; i1 < N1; i1++) {  // :1540-1556: keep what both directions agree on
        const int idx2 = vnMatch1[i1];
        if (idx2 >= 0) {
            const int idx1 = vnMatch2[idx2];
            if (idx1 == i1) {
                vnMatches12[i1] = idx2;
                nFound++;
            }
        }
    }
    return nFound;
}

// ORBmatcher.cc:515-643
int AMOS_VIEW_MATCHER::SearchForInitialization(const amos_frame_view &F1, const FeatureGrid &F2g, vector<cv::Point2f> &vbPrevMatched,
                                        vector<int> &vnMatches12, int windowSize)
{
    const amos_frame_view &F2 = F2g.Frame();
    int nmatches = 0;
    vnMatches12 = vector<int>(F1.n, -1);
    vector<int> vMatchedDistance(F2.n, INT_MAX);
    vector<int> vnMatches21(F2.n, -1);
    // every feature of F1 is a query, so F1.descriptors serves as the query block; only level 0 features get candidates (:540-552)
    CandidateLists c;
    for (int i1 = 0; i1 < F1.n; i1++) {
        const int level1 = F1.keys_un[i1].octave;
        c.Open();
        if (level1 <= 0) F2g.AppendFeaturesInArea(c.idx, vbPrevMatched[i1].x, vbPrevMatched[i1].y, windowSize, level1, level1);
    }
    c.Distances(*this, F2.descriptors, F2.n, F1.descriptors);
    RotationHistogram rotHist;
    for (int i1 = 0; i1 < F1.n; i1++) {
        if (F1.keys_un[i1].octave > 0) continue;
        if (c.Empty(i1)) continue;
        int bestDist = INT_MAX, bestDist2 = INT_MAX;
        const int bestIdx2 = c.Best2(i1, bestDist, bestDist2, [&](int i2, int d) { return vMatchedDistance[i2] <= d; });  // :554-555
        if (bestDist <= TH_LOW) {
            if (bestDist < (float)bestDist2 * mfNNratio) {
                if (vnMatches21[bestIdx2] >= 0) {  // displaces the earlier match of bestIdx2, whose vote stays in the histogram
                    vnMatches12[vnMatches21[bestIdx2]] = -1;
                    nmatches--;
                }
                vnMatches12[i1] = bestIdx2;
                vnMatches21[bestIdx2] = i1;
                vMatchedDistance[bestIdx2] = bestDist;
                nmatches++;
                if (mbCheckOrientation) rotHist.Add(F1.keys_un[i1].angle, F2.keys_un[bestIdx2].angle, i1);
            }
        }
    }
    if (mbCheckOrientation) nmatches -= rotHist.Prune(vnMatches12, -1, /*onlyIfSet=*/true);
    for (size_t i1 = 0, iend1 = vnMatches12.size(); i1 < iend1; i1++)
        if (vnMatches12[i1] >= 0) {
            vbPrevMatched[i1].x = F2.keys_un[vnMatches12[i1]].x;
            vbPrevMatched[i1].y = F2.keys_un[vnMatches12[i1]].y;
        }
    return nmatches;
}

// ORBmatcher.cc:1866-1908
void AMOS_VIEW_MATCHER::ComputeThreeMaxima(vector<int> *histo, const int L, int &ind1, int &ind2, int &ind3)
{
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < L; i++) {
        const int s = histo[i].size();
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            ind3 = ind2; ind2 = ind1; ind1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            ind3 = ind2; ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
}

}  // namespace ORB_SLAM2
