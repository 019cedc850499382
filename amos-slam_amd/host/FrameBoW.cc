// FrameBoW.cc -- host side of ORB_SLAM2::DeviceVocabulary, ComputeBoW and SearchByBoW: the text loader, and the calls of the C ABI on the
// vocabulary's handle and on the calling thread's matcher handle; nothing of the transform or the search is computed here.
#include "FrameBoW.h"

#include <cstdlib>
#include <fstream>
#include <sstream>

#include "FrameLocalPoints.h"  // ThreadMatcherHandle

namespace ORB_SLAM2
{

DeviceVocabulary::~DeviceVocabulary()
{
    if (handle_) amos_bow_destroy(handle_);
}

int DeviceVocabulary::fail(const std::string &what)
{
    parent_.clear(); isLeaf_.clear(); desc_.clear(); weight_.clear();
    nWords_ = 0;
    error_ = what;
    return status_ = AMOS_ERR_INVALID;
}

bool DeviceVocabulary::loadFromTextFile(const std::string &filename)
{
    std::lock_guard<std::mutex> lock(mutex_);
    if (handle_) { amos_bow_destroy(handle_); handle_ = nullptr; }
    status_ = AMOS_OK;
    error_.clear();
    std::ifstream f(filename.c_str());
    if (!f) return fail("cannot open " + filename) == AMOS_OK;
    std::string s;
    if (!std::getline(f, s)) return fail(filename + ": empty file") == AMOS_OK;
    {
        std::istringstream ss(s);
        std::string rest;
        if (!(ss >> k_ >> L_ >> scoring_ >> weighting_) || (ss >> rest)) return fail(filename + ": the first line is not 'k L scoring weighting'") == AMOS_OK;
    }
    parent_.assign(1, 0); isLeaf_.assign(1, 0); desc_.assign(32, 0); weight_.assign(1, 0.0);  // the root
    for (size_t line = 2; std::getline(f, s); line++) {
        if (s.find_first_not_of(" \t\r") == std::string::npos) continue;
        std::istringstream ss(s);
        long pid, leaf, byte;
        double w;
        std::string rest;
        const std::string where = filename + ":" + std::to_string(line);
        if (!(ss >> pid >> leaf)) return fail(where + ": parent id and leaf flag expected") == AMOS_OK;
        if (pid < 0 || pid >= (long)parent_.size()) return fail(where + ": parent " + std::to_string(pid) + " is not an earlier node") == AMOS_OK;
        uint8_t d[32];
        for (int i = 0; i < 32; i++) {
            if (!(ss >> byte) || byte < 0 || byte > 255) return fail(where + ": 32 descriptor bytes 0 .. 255 expected") == AMOS_OK;
            d[i] = (uint8_t)byte;
        }
        if (!(ss >> w) || (ss >> rest)) return fail(where + ": one weight expected after the descriptor") == AMOS_OK;
        parent_.push_back((int32_t)pid);
        isLeaf_.push_back(leaf > 0 ? 1 : 0);  // :1408
        desc_.insert(desc_.end(), d, d + 32);
        weight_.push_back(w);
    }
    int32_t words = 0;
    if (amos_bow_check(k_, L_, scoring_, weighting_, (int)parent_.size(), parent_.data(), isLeaf_.data(), &words) != AMOS_OK)
        return fail(filename + ": " + amos_last_error()) == AMOS_OK;
    nWords_ = words;
    return true;
}

int DeviceVocabulary::transformArrays(const uint8_t *descriptors, int n, int levelsup, Flat &out)
{
    std::lock_guard<std::mutex> lock(mutex_);
    if (parent_.size() < 2) { error_ = "the vocabulary is empty"; return AMOS_ERR_STATE; }
    if (!handle_) {
        const char *env = std::getenv("AMOS_DEVICE");
        const int device = env ? std::atoi(env) : amos_current_device();
        if (device < 0) return AMOS_ERR_DEVICE;
        const int rc = amos_bow_create(device, nullptr, k_, L_, scoring_, weighting_, (int)parent_.size(), parent_.data(), isLeaf_.data(),
                                       desc_.data(), weight_.data(), &handle_);
        if (rc != AMOS_OK) { handle_ = nullptr; return rc; }
    }
    const size_t m = (size_t)(n > 0 ? n : 0);
    out.featWord.resize(m); out.featNode.resize(m); out.nodeIds.resize(m); out.words.resize(m);
    out.nodeOff.resize(m + 1); out.nodeIdx.resize(m); out.wordWeights.resize(m);
    return amos_bow_transform(handle_, descriptors, n, levelsup, out.featWord.data(), out.featNode.data(), out.nodeIds.data(), out.nodeOff.data(),
                              out.nodeIdx.data(), out.words.data(), out.wordWeights.data(), &out.stats);
}

int SearchByBoWViews(const amos_bow_view &kf, const amos_bow_view &f, float nnratio, bool checkOri, int32_t *matchesF, amos_bow_search_stats *stats)
{
    amos_match *h = ThreadMatcherHandle();
    if (!h) return -1;
    if (amos_match_bow(h, &kf, &f, nnratio, checkOri ? 1 : 0, matchesF, stats) != AMOS_OK) return -1;
    return stats->n_matches;
}

}  // namespace ORB_SLAM2
