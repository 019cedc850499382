// amos_match_core.h -- what the matcher's source files share (amos_match.hip, amos_local.hip, amos_motion.hip): the 256-bit descriptor with
// its load and popcount, the best / second-best key reduction, the cell-range arithmetic of Frame::GetFeaturesInArea (Frame.cc:913-939), the
// wave-wide search of one window, and the matcher handle with its staging helpers.
#pragma once
#include "amos_common.h"

#include <algorithm>
#include <cstring>

namespace amos {

struct Desc {
    uint32_t w[8];
};

__device__ __forceinline__ int hamming256(const Desc &a, const Desc &b)
{
    int d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d += __popc(a.w[i] ^ b.w[i]);
    return d;
}

__device__ __forceinline__ Desc load_desc(const uint8_t *p)
{
    Desc d;
    const uint4 lo = reinterpret_cast<const uint4 *>(p)[0], hi = reinterpret_cast<const uint4 *>(p)[1];
    d.w[0] = lo.x; d.w[1] = lo.y; d.w[2] = lo.z; d.w[3] = lo.w;
    d.w[4] = hi.x; d.w[5] = hi.y; d.w[6] = hi.z; d.w[7] = hi.w;
    return d;
}

// the same for a descriptor that is only 4-byte aligned (a field of a record)
__device__ __forceinline__ Desc load_desc_words(const uint8_t *p)
{
    Desc d;
#pragma unroll
    for (int i = 0; i < 8; i++) d.w[i] = reinterpret_cast<const uint32_t *>(p)[i];
    return d;
}

// popcount(x) + acc in ONE instruction.  The compiler knows v_bcnt_u32_b32's accumulate operand but
// re-associates an 8-term sum into 8 x v_bcnt(.., 0) + 3 x v_add3; the chained form is 8 instructions.
__device__ __forceinline__ int bcnt_acc(uint32_t x, int acc)
{
    int r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// top-2 of unique keys
template <typename K>
__device__ __forceinline__ void top2_push(K &best, K &second, K key)
{
    const K hi = best > key ? best : key;
    best = best < key ? best : key;
    second = second < hi ? second : hi;
}
template <typename K>
__device__ __forceinline__ void top2_merge(K &best, K &second, K ob, K os)
{
    const K hi = best > ob ? best : ob;
    const K lo2 = second < os ? second : os;
    best = best < ob ? best : ob;
    second = hi < lo2 ? hi : lo2;
}

constexpr int kGridCells = AMOS_FRAME_GRID_COLS * AMOS_FRAME_GRID_ROWS;
constexpr int kWindowLanes = 8;  // lanes per query of the window searches: each takes every 8th grid column of the window

// Frame.cc:913-939: the cells a window of radius r around (u, v) touches, clamped to the grid.  The reference returns early when a
// clamp range is empty; without that a query projected far outside the bounds would index cellStart with y0 >= ROWS.  An empty window
// has x1 = -1 (no column to walk); the cells (ix, y0 .. y1) of a column are consecutive in the CSR.
struct CellRange {
    int x0, x1, y0, y1;
};
__device__ __forceinline__ CellRange cell_range(float u, float v, float r, float minX, float minY, float wInv, float hInv)
{
    CellRange c;
    c.x0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(u, minX), r), wInv));
    c.x1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(u, minX), r), wInv));
    c.y0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(v, minY), r), hInv));
    c.y1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(v, minY), r), hInv));
    const bool empty = c.x0 >= AMOS_FRAME_GRID_COLS || c.x1 < 0 || c.y0 >= AMOS_FRAME_GRID_ROWS || c.y1 < 0;
    c.x0 = max(c.x0, 0); c.y0 = max(c.y0, 0);
    c.x1 = empty ? -1 : min(c.x1, AMOS_FRAME_GRID_COLS - 1); c.y1 = min(c.y1, AMOS_FRAME_GRID_ROWS - 1);
    c.y0 = min(c.y0, AMOS_FRAME_GRID_ROWS - 1);
    return c;
}
// the item range [b, e) of column ix of the window in a frame's CSR
__device__ __forceinline__ void column_items(const int *cs, const CellRange &c, int ix, int &b, int &e)
{
    b = cs[ix * AMOS_FRAME_GRID_ROWS + c.y0];
    e = c.y1 >= c.y0 ? cs[ix * AMOS_FRAME_GRID_ROWS + c.y1 + 1] : b;
}

// The best two candidates of a window for a whole wave (the greedy loops of amos_local.hip and amos_motion.hip search a window again with
// it when the prepass record no longer holds).  All 64 lanes call it converged.  The window's columns (at most 64: the grid has 64) hold
// one item range each; lane l fetches the range of column x0 + l, an inclusive scan numbers the items of all columns 0 .. total - 1, and
// the lanes stride over THAT range: item t lies in the last column whose first number is <= t (a binary search over the lanes' exclusive
// sums).  cand(idx, j, key) says whether feature idx at CSR position j is a candidate and gives its key dist << 16 | j; best / second
// come back wave-uniform, 0xffffffff for none.
template <class Cand>
__device__ __forceinline__ void wave_window_best2(const int *cs, const int *it, const CellRange &c, int lane, Cand cand, unsigned &best, unsigned &second)
{
    best = second = 0xffffffffu;
    const int ncols = c.x1 - c.x0 + 1;
    int b = 0, e = 0;
    if (lane < ncols) column_items(cs, c, c.x0 + lane, b, e);
    const int cnt = e - b;
    int inc = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    const int total = __builtin_amdgcn_readlane(inc, 63), exc = inc - cnt;
    for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        int col = 0;
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) {  // col + step <= 63
            const int ev = __shfl(exc, col + step, 64);
            if (ev <= t) col += step;
        }
        const int cb = __shfl(b, col, 64), ce = __shfl(exc, col, 64);
        if (t < total) {
            const int j = cb + (t - ce);
            unsigned key;
            if (cand(it[j], j, key)) top2_push(best, second, key);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned ob = __shfl_xor(best, off, 64), os = __shfl_xor(second, off, 64);
        top2_merge(best, second, ob, os);
    }
    best = __builtin_amdgcn_readfirstlane(best);
    second = __builtin_amdgcn_readfirstlane(second);
}

}  // namespace amos

struct amos_match : amos::StreamHandle {
    // device scratch of the host-pointer entry points: the inputs of the call in flight (pointers into dArena), the grow-only result buffer
    uint8_t *dQ = nullptr, *dT = nullptr;
    int *dOff = nullptr, *dIdx = nullptr;
    void *dOut = nullptr;
    size_t capOut = 0;
    // pinned host staging of the host-buffer calls: the caller's (pageable) arrays are copied here and travel as true asynchronous DMA
    // transfers; results land here behind the kernel and are copied out after the ONE synchronisation of the call (a hipMemcpyAsync on
    // pageable memory is a blocking staged copy of its own: six of them were most of a 0.26 ms list-distance call)
    uint8_t *hStage = nullptr;
    uint8_t *dArena = nullptr;  // device mirror of the staging buffer's input part: the inputs of a call travel as ONE transfer (dQ / dT / dOff / dIdx point into it)
    size_t capStage = 0, stageUsed = 0;
    int bfKernel = 0;  // brute-force best-2: 0 = choose by size, 1 = xor + popcount kernel, 2 = i8 MFMA kernel
    // scratch of the local-map and motion-model searches (amos_local.hip, amos_motion.hip; calls are ordered on the stream): per-frame
    // parameters, best-two records and point flags of the call in flight
    uint8_t *dLocal = nullptr;
    size_t capLocal = 0;
    uint8_t *hLocal = nullptr;          // pinned: the per-frame parameters on their way to dLocal
    size_t capHLocal = 0;
    hipEvent_t localCopied = nullptr;   // recorded behind that copy
};

namespace amos {

template <typename T>
inline int grow(T **p, size_t *cap, size_t need)
{
    if (need <= *cap) return AMOS_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const size_t n = std::max<size_t>(need + need / 2, 256);
    AMOS_HIP_CHECK(hipMalloc((void **)p, n * sizeof(T)));
    *cap = n;
    return AMOS_OK;
}

// every host-buffer call ends with a stream synchronisation, so the staging buffer is free at the start of the next one
inline int stage_begin(amos_match *m, size_t bytes)
{
    m->stageUsed = 0;
    bytes += 1024;  // alignment slack of the pieces
    if (bytes <= m->capStage) return AMOS_OK;
    if (m->hStage || m->dArena) (void)hipStreamSynchronize(m->stream);  // (a call that failed half way may have left a transfer in flight)
    if (m->hStage) (void)hipHostFree(m->hStage);
    if (m->dArena) (void)hipFree(m->dArena);
    m->hStage = m->dArena = nullptr;
    m->capStage = 0;
    const size_t n = std::max<size_t>(bytes + bytes / 2, 1 << 16);
    if (hipHostMalloc((void **)&m->hStage, n, hipHostMallocDefault) != hipSuccess || hipMalloc((void **)&m->dArena, n) != hipSuccess) {
        (void)hipGetLastError();
        set_error("matcher staging of %zu bytes (pinned host + device) could not be allocated", n);
        return AMOS_ERR_DEVICE;
    }
    m->capStage = n;
    return AMOS_OK;
}

inline size_t stage_take(amos_match *m, size_t bytes)
{
    const size_t o = m->stageUsed;
    m->stageUsed += (bytes + 63) & ~(size_t)63;
    return o;  // (stage_begin sized the buffers for the sum of the call's pieces)
}

// host array -> staging; returns where it will sit on the device once stage_flush has run
template <typename T>
inline T *stage_input(amos_match *m, const void *src, size_t bytes)
{
    const size_t o = stage_take(m, bytes);
    if (bytes) std::memcpy(m->hStage + o, src, bytes);
    return reinterpret_cast<T *>(m->dArena + o);
}

inline int stage_flush(amos_match *m)
{
    if (m->stageUsed) AMOS_HIP_CHECK(hipMemcpyAsync(m->dArena, m->hStage, m->stageUsed, hipMemcpyHostToDevice, m->stream));
    return AMOS_OK;
}

// device -> staging (behind the inputs), one synchronisation, staging -> `out`
inline int stage_d2h_sync(amos_match *m, void *out, const void *src, size_t bytes)
{
    uint8_t *p = m->hStage + stage_take(m, bytes);
    AMOS_HIP_CHECK(hipMemcpyAsync(p, src, bytes, hipMemcpyDeviceToHost, m->stream));
    AMOS_HIP_CHECK(hipStreamSynchronize(m->stream));
    std::memcpy(out, p, bytes);
    return AMOS_OK;
}

inline int grow_out(amos_match *m, size_t bytes)
{
    uint8_t *p = (uint8_t *)m->dOut;
    int rc = grow(&p, &m->capOut, bytes);
    m->dOut = p;
    return rc;
}

}  // namespace amos
