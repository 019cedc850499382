// amos_mask_pre.hip -- the mask pass's pre-processing chain on the device: from the raw BGR
// frame to the network's input tensor, numerically what the reference does in three places -- as one kernel that keeps
// the two intermediate images in LDS (k_mask_pre_fused), or as three small kernels through HBM:
//   A  yolact::evalImage (yolact.cc:220, 385-451): cv::resize(BGR u8 -> W480 x H640) [sic, swapped], u8 / 255.0
//      as CHW float, and eval_image's "* 255" (yolact_interface.py:862-864)            -> float HWC 640 x 480
//   B  eval_image's cv2.resize(float32, (640, 480)) (yolact_interface.py:865)          -> float HWC 480 x 640
//   C  FastBaseTransform (utils/augmentations.py:616-657): bilinear to 550 x 550 (align_corners=False),
//      (x - MEANS) / STD in BGR order, channels swapped to RGB                         -> float CHW 3 x 550 x 550
// The two OpenCV resizes use host-built tap tables (8-bit: 11-bit fixed point; float32: float
// weights), the u8 -> float step is a 256-entry table made on the host with the reference's double division.
// PyTorch is not involved: the network consumes d_out directly.
#include "amos_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace amos {

constexpr int kNetSize = 550;            // cfg.max_size
constexpr int kMidW = kMaskMidW, kMidH = kMaskMidH;  // yolact.cc:220  cv::Size(480, 640)
constexpr int kBackW = 640, kBackH = 480;  // yolact_interface.py:865

struct FltTap { int s0, s1; float f0, f1; };  // float cv::resize: source indices, (1 - f) and f

// A: grid = (ceil(480 * 640 / 256), frames); one thread per intermediate pixel, three channels
__global__ __launch_bounds__(256) void k_mask_pre_a(const uint8_t *__restrict__ bgr, int srcW, int srcH, const FixTap *__restrict__ tx,
                                                   const FixTap *__restrict__ ty, const float *__restrict__ lut, float *__restrict__ mid)
{
    const int p = blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
    if (p >= kMidW * kMidH) return;
    const int y = p / kMidW, x = p - y * kMidW;
    const FixTap ax = tx[x], ay = ty[y];
    const uint8_t *r0 = bgr + ((size_t)frame * srcH + ay.s0) * srcW * 3, *r1 = bgr + ((size_t)frame * srcH + ay.s1) * srcW * 3;
    float *o = mid + ((size_t)frame * kMidH * kMidW + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int h0 = r0[ax.s0 * 3 + c] * ax.a0 + r0[ax.s1 * 3 + c] * ax.a1;
        const int h1 = r1[ax.s0 * 3 + c] * ax.a0 + r1[ax.s1 * 3 + c] * ax.a1;
        const int v = (((ay.a0 * (h0 >> 4)) >> 16) + ((ay.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
        o[c] = lut[v];  // float(double(v) / 255.0) * 255.0f
    }
}

// B: grid = (ceil(640 * 480 / 256), frames); cv::resize float INTER_LINEAR, horizontal then vertical, no FMA
__global__ __launch_bounds__(256) void k_mask_pre_b(const float *__restrict__ mid, const FltTap *__restrict__ tx, const FltTap *__restrict__ ty,
                                                   float *__restrict__ back)
{
    const int p = blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
    if (p >= kBackW * kBackH) return;
    const int y = p / kBackW, x = p - y * kBackW;
    const FltTap ax = tx[x], ay = ty[y];
    const float *r0 = mid + ((size_t)frame * kMidH + ay.s0) * kMidW * 3, *r1 = mid + ((size_t)frame * kMidH + ay.s1) * kMidW * 3;
    float *o = back + ((size_t)frame * kBackH * kBackW + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float h0 = __fadd_rn(__fmul_rn(r0[ax.s0 * 3 + c], ax.f0), __fmul_rn(r0[ax.s1 * 3 + c], ax.f1));
        const float h1 = __fadd_rn(__fmul_rn(r1[ax.s0 * 3 + c], ax.f0), __fmul_rn(r1[ax.s1 * 3 + c], ax.f1));
        o[c] = __fadd_rn(__fmul_rn(h0, ay.f0), __fmul_rn(h1, ay.f1));
    }
}

// C: grid = (ceil(550 * 550 / 256), frames); torch.nn.functional.interpolate(bilinear, align_corners=False),
// normalisation and the BGR -> RGB swap; writes planar CHW
__global__ __launch_bounds__(256) void k_mask_pre_c(const float *__restrict__ back, float *__restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
    if (p >= kNetSize * kNetSize) return;
    const int oy = p / kNetSize, ox = p - oy * kNetSize;
    const float sh = (float)kBackH / (float)kNetSize, sw = (float)kBackW / (float)kNetSize;
    const float hr = fmaxf(__fsub_rn(__fmul_rn(sh, __fadd_rn((float)oy, 0.5f)), 0.5f), 0.f);
    const float wr = fmaxf(__fsub_rn(__fmul_rn(sw, __fadd_rn((float)ox, 0.5f)), 0.5f), 0.f);
    const int h1 = (int)hr, w1 = (int)wr;
    const int h1p = h1 < kBackH - 1 ? 1 : 0, w1p = w1 < kBackW - 1 ? 1 : 0;
    const float hl1 = __fsub_rn(hr, (float)h1), hl0 = __fsub_rn(1.f, hl1);
    const float wl1 = __fsub_rn(wr, (float)w1), wl0 = __fsub_rn(1.f, wl1);
    const float *b = back + (size_t)frame * kBackH * kBackW * 3;
    const float *p00 = b + ((size_t)h1 * kBackW + w1) * 3, *p01 = p00 + w1p * 3, *p10 = p00 + (size_t)h1p * kBackW * 3, *p11 = p10 + w1p * 3;
    const float mean[3] = {103.94f, 116.78f, 123.68f}, stdv[3] = {57.38f, 57.12f, 58.40f};  // BGR, data/config.py:28-29
    float *o = out + (size_t)frame * 3 * kNetSize * kNetSize + p;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float top = __fadd_rn(__fmul_rn(wl0, p00[c]), __fmul_rn(wl1, p01[c]));
        const float bot = __fadd_rn(__fmul_rn(wl0, p10[c]), __fmul_rn(wl1, p11[c]));
        const float v = __fadd_rn(__fmul_rn(hl0, top), __fmul_rn(hl1, bot));
        o[(size_t)(2 - c) * kNetSize * kNetSize] = __fdiv_rn(__fsub_rn(v, mean[c]), stdv[c]);  // RGB plane order
    }
}


// The three stages in ONE pass (amos_mask_pre_mode 1, the default): a work-group owns a kPreTile x kPreTile tile of network-input pixels and
// walks the chain backwards through the tap tables to the windows it needs -- stage C's taps of the tile's first and last row / column
// give the window of B, the B taps of that window's ends (dFltX / dFltY) the window of A, the A taps of its ends (dFixX / dFixY) the
// source window; every table is non-decreasing in both taps (checked on the host), so an inner element's taps lie inside.  The source
// window is staged in LDS, then A's window is computed into LDS once, B's from it, C from that: 0.29 GB per 64 frames (59 MB of frames in,
// 232 MB out) instead of 1.23 GB through the two 236 MB intermediates.  Every value is made by k_mask_pre_a / _b / _c's operations in
// their order: the same bits.
// LDS: B's and A's windows do not depend on the frame size (30 x 39 and 41 x 31 pixels of three floats: 14.0 + 15.3 KB; B's lies over the
// source window, which is dead by then); the source
// window does -- 32 x 42 pixels (4 KB) at 640 x 480, 47 x 82 (11.7 KB) at 1280 x 720 -- and gets kPreSrcBytes.  RULE: a frame size takes
// this kernel iff (most source rows of a tile) x pre_src_pitch(most source columns of a tile) is at most kPreSrcBytes (and the A / B
// windows are within their arrays); otherwise -- strong downscaling: 70 x 368 = 25.8 KB at 1920 x 1080 -- the three-kernel chain runs.
// The host evaluates the rule at create time over every tile with the kernel's own window arithmetic (pre_axis_window below).
// grid = (ceil(550 / 32), ceil(550 / 32), frames), block = 256.
constexpr int kPreTile = 32, kPreBRows = 30, kPreBCols = 39, kPreARows = 41, kPreACols = 31, kPreSrcBytes = 16 * 1024;

__host__ __device__ inline int pre_src_pitch(int cols) { return (cols * 3 + 3) & ~3; }  // bytes of a staged source row: three per pixel, whole dwords

struct PreTables { const FixTap *fixX, *fixY; const FltTap *fltX, *fltY; const float *lut; };

// stage C's tap of output index o (k_mask_pre_c's expressions): first source index, 0 / 1 step to the second, weights
__host__ __device__ inline void pre_c_tap(int o, float scale, int inN, int &i0, int &step, float &l0, float &l1)
{
#ifdef __HIP_DEVICE_COMPILE__
    const float r = fmaxf(__fsub_rn(__fmul_rn(scale, __fadd_rn((float)o, 0.5f)), 0.5f), 0.f);
    i0 = (int)r; step = i0 < inN - 1 ? 1 : 0;
    l1 = __fsub_rn(r, (float)i0); l0 = __fsub_rn(1.f, l1);
#else
    volatile float a = (float)o + 0.5f, b = scale * a, c = b - 0.5f;  // (volatile: one rounding per operation on the host too)
    const float r = c > 0.f ? c : 0.f;
    i0 = (int)r; step = i0 < inN - 1 ? 1 : 0;
    l1 = r - (float)i0; l0 = 1.f - l1;
#endif
}

// The windows of one tile along one axis: output indices [o0, o1] -> B's [b0, b1] -> A's [m0, m1] -> source [s0, s1]
struct PreAxisWindow { int b0, b1, m0, m1, s0, s1; };
__host__ __device__ inline PreAxisWindow pre_axis_window(int o0, int o1, int backN, float scale, const FltTap *flt, const FixTap *fix)
{
    PreAxisWindow w;
    int i, st;
    float l0, l1;
    pre_c_tap(o0, scale, backN, i, st, l0, l1);
    w.b0 = i;
    pre_c_tap(o1, scale, backN, i, st, l0, l1);
    w.b1 = i + st;
    w.m0 = flt[w.b0].s0; w.m1 = flt[w.b1].s1;
    w.s0 = fix[w.m0].s0; w.s1 = fix[w.m1].s1;
    return w;
}

__global__ __launch_bounds__(256) void k_mask_pre_fused(const uint8_t *__restrict__ src, size_t frameStride, size_t rowStride, int channels,
                                                       const PreTables t, float *__restrict__ out)
{
    __shared__ __align__(16) uint8_t sSrc[kPreSrcBytes];
    __shared__ float sA[kPreARows * kPreACols * 3];
    __shared__ float sLut[256];
    static_assert(kPreBRows * kPreBCols * 3 * sizeof(float) <= kPreSrcBytes, "B's window takes the source window's place");
    float *sB = reinterpret_cast<float *>(sSrc);  // the source window is dead once A is made (the barrier after stage A): 32.7 KB, five groups per CU
    const int tid = threadIdx.x, frame = blockIdx.z;
    const int ox0 = blockIdx.x * kPreTile, oy0 = blockIdx.y * kPreTile;
    const float sh = (float)kBackH / (float)kNetSize, sw = (float)kBackW / (float)kNetSize;
    const PreAxisWindow wx = pre_axis_window(ox0, min(ox0 + kPreTile, kNetSize) - 1, kBackW, sw, t.fltX, t.fixX);
    const PreAxisWindow wy = pre_axis_window(oy0, min(oy0 + kPreTile, kNetSize) - 1, kBackH, sh, t.fltY, t.fixY);
    const int nSC = wx.s1 - wx.s0 + 1, nSR = wy.s1 - wy.s0 + 1, pitch = pre_src_pitch(nSC);
    const int nAC = wx.m1 - wx.m0 + 1, nAR = wy.m1 - wy.m0 + 1, nBC = wx.b1 - wx.b0 + 1, nBR = wy.b1 - wy.b0 + 1;
    // idx / n for the window loops: one multiplication (m = floor((2^32 - 1) / n) + 1 is exact while idx * n < 2^32; idx < 2^13, n < 2^12);
    // n = 1 has no 32-bit m and is marked by 0
    auto magic = [](int n) { return n > 1 ? 0xffffffffu / (unsigned)n + 1u : 0u; };
    auto div = [](int idx, unsigned m) { return m ? (int)__umulhi((unsigned)idx, m) : idx; };
    sLut[tid] = t.lut[tid];
    const uint8_t *s0 = src + (size_t)frame * frameStride + (size_t)wy.s0 * rowStride + (size_t)wx.s0 * channels;
    if (channels == 3) {  // a window row is one run of bytes: four at a time (the tail, which may end the allocation, byte by byte)
        const int nb = nSC * 3, nd = pitch >> 2;
        const unsigned m = magic(nd);
        for (int idx = tid; idx < nSR * nd; idx += 256) {
            const int r = div(idx, m), j = 4 * (idx - r * nd);
            const uint8_t *g = s0 + (size_t)r * rowStride + j;
            unsigned v = 0;
            if (j + 4 <= nb) __builtin_memcpy(&v, g, 4);  // unaligned global_load_dword
            else
                for (int k = 0; j + k < nb; k++) v |= (unsigned)g[k] << (8 * k);
            *reinterpret_cast<unsigned *>(sSrc + r * pitch + j) = v;
        }
    } else {  // four bytes per pixel: one load, the first three kept
        const unsigned m = magic(nSC);
        for (int idx = tid; idx < nSR * nSC; idx += 256) {
            const int r = div(idx, m), c = idx - r * nSC;
            unsigned v;
            __builtin_memcpy(&v, s0 + (size_t)r * rowStride + (size_t)c * 4, 4);
            uint8_t *d = sSrc + r * pitch + 3 * c;
            d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16);
        }
    }
    __syncthreads();
    // Stages A, B and C keep one coordinate of a thread fixed over its loop, so that coordinate's taps, offsets and weights are made once:
    // A: 32 lanes = the window's columns (at most kPreACols = 31), 8 rows per pass
    static_assert(kPreACols <= 32 && kPreBRows <= 32 && kPreTile == 32, "the thread layouts below");
    const int lo = tid & 31, hi = tid >> 5;
    if (lo < nAC) {  // stage A, as k_mask_pre_a
        const FixTap ax = t.fixX[wx.m0 + lo];
        const int xa = 3 * (ax.s0 - wx.s0), xb = 3 * (ax.s1 - wx.s0);
        for (int r = hi; r < nAR; r += 8) {
            const FixTap ay = t.fixY[wy.m0 + r];
            const uint8_t *r0 = sSrc + (ay.s0 - wy.s0) * pitch, *r1 = sSrc + (ay.s1 - wy.s0) * pitch;
            float *o = sA + (r * nAC + lo) * 3;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int h0 = r0[xa + k] * ax.a0 + r0[xb + k] * ax.a1;
                const int h1 = r1[xa + k] * ax.a0 + r1[xb + k] * ax.a1;
                const int v = (((ay.a0 * (h0 >> 4)) >> 16) + ((ay.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
                o[k] = sLut[v];
            }
        }
    }
    __syncthreads();
    if (lo < nBR) {  // stage B, as k_mask_pre_b: 32 lanes = the window's rows (at most kPreBRows = 30), 8 columns per pass
        const FltTap ay = t.fltY[wy.b0 + lo];
        const float *r0 = sA + (ay.s0 - wy.m0) * nAC * 3, *r1 = sA + (ay.s1 - wy.m0) * nAC * 3;
        for (int c = hi; c < nBC; c += 8) {
            const FltTap ax = t.fltX[wx.b0 + c];
            const int xa = 3 * (ax.s0 - wx.m0), xb = 3 * (ax.s1 - wx.m0);
            float *o = sB + (lo * nBC + c) * 3;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float h0 = __fadd_rn(__fmul_rn(r0[xa + k], ax.f0), __fmul_rn(r0[xb + k], ax.f1));
                const float h1 = __fadd_rn(__fmul_rn(r1[xa + k], ax.f0), __fmul_rn(r1[xb + k], ax.f1));
                o[k] = __fadd_rn(__fmul_rn(h0, ay.f0), __fmul_rn(h1, ay.f1));
            }
        }
    }
    __syncthreads();
    const int ox = ox0 + lo;
    if (ox < kNetSize) {  // stage C, as k_mask_pre_c: 32 lanes = the tile's columns, 8 rows per pass
        const float mean[3] = {103.94f, 116.78f, 123.68f}, stdv[3] = {57.38f, 57.12f, 58.40f};  // BGR, data/config.py:28-29
        int w1, w1p;
        float wl0, wl1;
        pre_c_tap(ox, sw, kBackW, w1, w1p, wl0, wl1);
        const float *col = sB + (w1 - wx.b0) * 3;
        for (int oy = oy0 + hi; oy < min(oy0 + kPreTile, kNetSize); oy += 8) {
            int h1, h1p;
            float hl0, hl1;
            pre_c_tap(oy, sh, kBackH, h1, h1p, hl0, hl1);
            const float *p00 = col + (h1 - wy.b0) * nBC * 3, *p01 = p00 + w1p * 3, *p10 = p00 + h1p * nBC * 3, *p11 = p10 + w1p * 3;
            float *o = out + (size_t)frame * 3 * kNetSize * kNetSize + (size_t)oy * kNetSize + ox;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float top = __fadd_rn(__fmul_rn(wl0, p00[k]), __fmul_rn(wl1, p01[k]));
                const float bot = __fadd_rn(__fmul_rn(wl0, p10[k]), __fmul_rn(wl1, p11[k]));
                const float v = __fadd_rn(__fmul_rn(hl0, top), __fmul_rn(hl1, bot));
                o[(size_t)(2 - k) * kNetSize * kNetSize] = __fdiv_rn(__fsub_rn(v, mean[k]), stdv[k]);  // RGB plane order
            }
        }
    }
}


// ---- epilogue of a convolution of the mask network, fused: y = act(y + bias[c] (+ residual)), in place, on an NHWC
// (channels-last) float tensor.  MIOpen's convolutions take no bias and PyTorch adds it, the residual and the ReLU as
// one elementwise pass each over the activations (three reads + three writes of the tensor per bottleneck output);
// this is one read (+ the residual) and one write.  Sums in the order (y + b) + r, like the unfused ops: same bits.
// grid = ceil(n / 4 / 256), block = 256; kVec: channels % 4 == 0 and 16-byte aligned pointers; kPow2: channels is a
// power of two (every ResNet / FPN width), so the channel of an element is a mask, not a 64-bit modulo.
template <bool kVec, bool kPow2>
__global__ __launch_bounds__(256) void k_bias_act(float *__restrict__ y, const float *__restrict__ bias, const float *__restrict__ res, size_t n,
                                                 int channels, int relu)
{
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (kVec) {
        const unsigned c = kPow2 ? ((unsigned)i & (unsigned)(channels - 1)) : (unsigned)(i % (size_t)channels);
        float4 v = *reinterpret_cast<const float4 *>(y + i);
        const float4 b = *reinterpret_cast<const float4 *>(bias + c);
        v.x = __fadd_rn(v.x, b.x); v.y = __fadd_rn(v.y, b.y); v.z = __fadd_rn(v.z, b.z); v.w = __fadd_rn(v.w, b.w);
        if (res) {
            const float4 r = *reinterpret_cast<const float4 *>(res + i);
            v.x = __fadd_rn(v.x, r.x); v.y = __fadd_rn(v.y, r.y); v.z = __fadd_rn(v.z, r.z); v.w = __fadd_rn(v.w, r.w);
        }
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        *reinterpret_cast<float4 *>(y + i) = v;
    } else {
        for (size_t k = i; k < n && k < i + 4; k++) {
            float v = __fadd_rn(y[k], bias[k % (size_t)channels]);
            if (res) v = __fadd_rn(v, res[k]);
            y[k] = relu ? fmaxf(v, 0.f) : v;
        }
    }
}

// The same resize for an exact x 2 enlargement (the prototype network's upsampling step: 256 channels, 69 -> 138, 1.25 GB written per 64
// frames): a thread makes the 2 x 2 output block around one source pixel from the 3 x 3 source pixels it touches -- 2.25 sixteen-byte
// reads per output instead of 4 (the one-output-per-thread kernel above moves 10 TB/s from L2 to L1 for this layer and is bound by that).
// Per output the same taps, weights and order of operations as k_bilinear_nhwc: the same bits.  A block whose two rows (columns) do not
// share their middle source row (column) -- the first and last ones, where the source index is clamped -- takes its taps one by one.
// grid = (ceil(ceil(outH / 2) * ceil(outW / 2) * c4 / 256), 1, n): the blocks of an image are numbered row by row, so a narrow image (the
// channel-blocked layout is images of 8 channels: 138 threads per block row) still fills its work-groups
template <bool kRelu>
__global__ __launch_bounds__(256) void k_bilinear_nhwc_x2(const float *__restrict__ x, float *__restrict__ y, int inH, int inW, int outH, int outW, int c4,
                                                         float scaleH, float scaleW)
{
    const int t = blockIdx.x * 256 + threadIdx.x, bw = (outW + 1) / 2, bh = (outH + 1) / 2, perRow = bw * c4;
    if (t >= bh * perRow) return;
    const int by = t / perRow, tr = t - by * perRow;
    const int bx = tr / c4, q = tr - bx * c4, n = blockIdx.z;
    int yy[2][2], xx[2][2];
    float wy[2][2], wx[2][2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        float fy = __fsub_rn(__fmul_rn(scaleH, __fadd_rn((float)(2 * by + e), 0.5f)), 0.5f);
        float fx = __fsub_rn(__fmul_rn(scaleW, __fadd_rn((float)(2 * bx + e), 0.5f)), 0.5f);
        fy = fy < 0.f ? 0.f : fy;
        fx = fx < 0.f ? 0.f : fx;
        yy[e][0] = min((int)fy, inH - 1);  // (only a row / column past the output, never stored, can exceed the source)
        xx[e][0] = min((int)fx, inW - 1);
        yy[e][1] = yy[e][0] + (yy[e][0] < inH - 1 ? 1 : 0);
        xx[e][1] = xx[e][0] + (xx[e][0] < inW - 1 ? 1 : 0);
        wy[e][1] = __fsub_rn(fy, (float)(int)fy); wy[e][0] = __fsub_rn(1.f, wy[e][1]);
        wx[e][1] = __fsub_rn(fx, (float)(int)fx); wx[e][0] = __fsub_rn(1.f, wx[e][1]);
    }
    const float4 *src = reinterpret_cast<const float4 *>(x) + (size_t)n * inH * inW * c4;
    auto at = [&](int r, int c) { return src[((size_t)r * inW + c) * c4 + q]; };
    float4 s[4][4];  // [row tap: a0 a1 b0 b1][column tap: a0 a1 b0 b1]
    const bool shareY = yy[1][0] == yy[0][1], shareX = xx[1][0] == xx[0][1];
    const int ry[4] = {yy[0][0], yy[0][1], yy[1][0], yy[1][1]}, cx[4] = {xx[0][0], xx[0][1], xx[1][0], xx[1][1]};
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (r == 2 && shareY) {
#pragma unroll
            for (int c = 0; c < 4; c++) s[2][c] = s[1][c];
            continue;
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (c == 2 && shareX) s[r][2] = s[r][1];
            else s[r][c] = at(ry[r], cx[c]);
        }
    }
    float4 *dst = reinterpret_cast<float4 *>(y);
#pragma unroll
    for (int ey = 0; ey < 2; ey++)
#pragma unroll
        for (int ex = 0; ex < 2; ex++) {
            const int oy = 2 * by + ey, ox = 2 * bx + ex;
            if (oy >= outH || ox >= outW) continue;
            const float hy = wy[ey][0], ly = wy[ey][1], hx = wx[ex][0], lx = wx[ex][1];
            const float4 a = s[2 * ey][2 * ex], b = s[2 * ey][2 * ex + 1], c = s[2 * ey + 1][2 * ex], d = s[2 * ey + 1][2 * ex + 1];
            auto mix = [&](float p, float r, float u, float v2) {
                const float v = __fadd_rn(__fmul_rn(hy, __fadd_rn(__fmul_rn(hx, p), __fmul_rn(lx, r))), __fmul_rn(ly, __fadd_rn(__fmul_rn(hx, u), __fmul_rn(lx, v2))));
                return kRelu ? (v < 0.f ? 0.f : v) : v;
            };
            dst[(((size_t)n * outH + oy) * outW + ox) * c4 + q] = make_float4(mix(a.x, b.x, c.x, d.x), mix(a.y, b.y, c.y, d.y), mix(a.z, b.z, c.z, d.z), mix(a.w, b.w, c.w, d.w));
        }
}

// ---- the stem's tail: bias + ReLU + max_pool2d(3, stride 2, padding 1) of the 7 x 7 convolution's raw output in one pass
// (backbone.py ResNetBackbone.forward: conv1 -> bn1 (folded) -> relu -> maxpool).  relu(x + b) is monotone in x, and rounding is
// monotone, so max over the window of relu(x_i + b) == relu(max_i(x_i) + b) bit for bit: the kernel takes the maximum of the raw
// values (padding = -inf, as F.max_pool2d pads) and applies bias and ReLU once.  Replaces the in-place bias/ReLU pass over the
// 275 x 275 x 64 tensor (read + write) and the pooling kernel's read of it with one read.
// grid = (ceil(outW * C / 4 / 256), outH, N), block = 256; a thread makes four channels of one pooled pixel.
__global__ __launch_bounds__(256) void k_bias_relu_maxpool(const float *__restrict__ x, const float *__restrict__ bias, float *__restrict__ y, int inH, int inW,
                                                          int outH, int outW, int c4)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= outW * c4) return;
    const int ox = t / c4, q = t - ox * c4, oy = blockIdx.y, n = blockIdx.z;
    const float4 *src = reinterpret_cast<const float4 *>(x) + (size_t)n * inH * inW * c4;
    const float ninf = -__builtin_inff();
    float4 m = {ninf, ninf, ninf, ninf};
    bool nan = false;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int iy = 2 * oy + dy;
        if ((unsigned)iy >= (unsigned)inH) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int ix = 2 * ox + dx;
            if ((unsigned)ix >= (unsigned)inW) continue;
            const float4 v = src[((size_t)iy * inW + ix) * c4 + q];
            nan = nan || v.x != v.x || v.y != v.y || v.z != v.z || v.w != v.w;
            m.x = v.x > m.x ? v.x : m.x; m.y = v.y > m.y ? v.y : m.y; m.z = v.z > m.z ? v.z : m.z; m.w = v.w > m.w ? v.w : m.w;
        }
    }
    const float4 b = reinterpret_cast<const float4 *>(bias)[q];
    float4 r = {fmaxf(__fadd_rn(m.x, b.x), 0.f), fmaxf(__fadd_rn(m.y, b.y), 0.f), fmaxf(__fadd_rn(m.z, b.z), 0.f), fmaxf(__fadd_rn(m.w, b.w), 0.f)};
    if (nan) {  // rare path: per component, a NaN in the window wins (as in max_pool2d of the relu'd tensor)
        float *rp = &r.x;
        for (int e = 0; e < 4; e++) {
            bool cn = false;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int iy = 2 * oy + dy, ix = 2 * ox + dx;
                    if ((unsigned)iy < (unsigned)inH && (unsigned)ix < (unsigned)inW) {
                        const float v = (&src[((size_t)iy * inW + ix) * c4 + q].x)[e];
                        cn = cn || v != v;
                    }
                }
            if (cn) rp[e] = __builtin_nanf("");
        }
    }
    reinterpret_cast<float4 *>(y)[(((size_t)n * outH + oy) * outW + ox) * c4 + q] = r;
}

// ---- bilinear resize of an NHWC float tensor (F.interpolate(..., mode="bilinear", align_corners=False): the FPN's
// top-down path and the prototype network's x2 step, yolact.py:318-329, config mask_proto_net).  PyTorch's channels-last
// kernel for this took 13 % of the mask pass (5 ms per call at 32 frames); here a thread makes four channels of one
// output pixel with 16-byte loads / stores.  Source index and weights as PyTorch computes them in float32:
// src = scale * (dst + 0.5) - 0.5, clamped at 0, scale = 1 / scale_factor when given, else in / out.
// grid = (ceil(outW * C / 4 / 256), outH, N), block = 256.
template <bool kRelu>
__global__ __launch_bounds__(256) void k_bilinear_nhwc(const float *__restrict__ x, float *__restrict__ y, int inH, int inW, int outH, int outW, int c4,
                                                      float scaleH, float scaleW)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= outW * c4) return;
    const int ox = t / c4, q = t - ox * c4, oy = blockIdx.y, n = blockIdx.z;
    float fy = __fsub_rn(__fmul_rn(scaleH, __fadd_rn((float)oy, 0.5f)), 0.5f), fx = __fsub_rn(__fmul_rn(scaleW, __fadd_rn((float)ox, 0.5f)), 0.5f);
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < inH - 1 ? 1 : 0), x1 = x0 + (x0 < inW - 1 ? 1 : 0);
    const float ly = __fsub_rn(fy, (float)y0), lx = __fsub_rn(fx, (float)x0), hy = __fsub_rn(1.f, ly), hx = __fsub_rn(1.f, lx);
    const float4 *src = reinterpret_cast<const float4 *>(x) + (size_t)n * inH * inW * c4;
    const float4 a = src[((size_t)y0 * inW + x0) * c4 + q], b = src[((size_t)y0 * inW + x1) * c4 + q];
    const float4 c = src[((size_t)y1 * inW + x0) * c4 + q], d = src[((size_t)y1 * inW + x1) * c4 + q];
    auto mix = [&](float p, float r, float s, float u) {  // h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)
        const float v = __fadd_rn(__fmul_rn(hy, __fadd_rn(__fmul_rn(hx, p), __fmul_rn(lx, r))), __fmul_rn(ly, __fadd_rn(__fmul_rn(hx, s), __fmul_rn(lx, u))));
        return kRelu ? (v < 0.f ? 0.f : v) : v;  // a NaN stays a NaN, as through torch.relu
    };
    reinterpret_cast<float4 *>(y)[(((size_t)n * outH + oy) * outW + ox) * c4 + q] =
        make_float4(mix(a.x, b.x, c.x, d.x), mix(a.y, b.y, c.y, d.y), mix(a.z, b.z, c.z, d.z), mix(a.w, b.w, c.w, d.w));
}

// Fast NMS suppression term (layers/functions/detection.py:103-170 fast_nms as mask/detect.py restates it): for every class list of
// k score-sorted boxes, out[j] = max over i < j of IoU(box i, box j) (the column maxima of the upper-triangular IoU matrix; 0 for
// j = 0).  PyTorch spends nine elementwise passes over the [lists][k][k] matrix on this (410 MB at 32 frames x 80 classes x 200);
// here a work-group keeps one list's boxes in LDS and every thread walks its column.  box_utils.jaccard's arithmetic in its order:
// intersection = clamp(min(x2) - max(x1), 0) * clamp(min(y2) - max(y1), 0); IoU = inter / ((area_i + area_j) - inter), correctly
// rounded; a NaN (0 / 0) wins the maximum as it does in torch.max.
// grid = lists, block = 256 (k <= 256).
__global__ __launch_bounds__(256) void k_nms_column_max(const float4 *__restrict__ boxes, float *__restrict__ out, int k)
{
    __shared__ float4 sb[256];
    __shared__ float sarea[256];
    const int j = threadIdx.x;
    const float4 *b = boxes + (size_t)blockIdx.x * k;
    float4 me = {0.f, 0.f, 0.f, 0.f};
    float myArea = 0.f;
    if (j < k) {
        me = b[j];
        myArea = __fmul_rn(__fsub_rn(me.z, me.x), __fsub_rn(me.w, me.y));
        sb[j] = me;
        sarea[j] = myArea;
    }
    __syncthreads();
    if (j >= k) return;
    float best = 0.f;
    bool nan = false;
    for (int i = 0; i < j; i++) {
        const float4 o = sb[i];  // the same address for every lane: a broadcast
        float w = __fsub_rn(fminf(o.z, me.z), fmaxf(o.x, me.x)), h = __fsub_rn(fminf(o.w, me.w), fmaxf(o.y, me.y));
        w = w < 0.f ? 0.f : w;
        h = h < 0.f ? 0.f : h;
        const float inter = __fmul_rn(w, h);
        const float uni = __fsub_rn(__fadd_rn(sarea[i], myArea), inter);
        const float iou = (float)((double)inter / (double)uni);  // == the correctly rounded float quotient
        nan = nan || iou != iou;
        best = iou > best ? iou : best;
    }
    out[(size_t)blockIdx.x * k + j] = nan ? __builtin_nanf("") : best;
}

}  // namespace amos

using namespace amos;

struct amos_mask_pre : StreamHandle {
    int width = 0, height = 0, maxBatch = 0;
    FixTap *dFixX = nullptr, *dFixY = nullptr;
    FltTap *dFltX = nullptr, *dFltY = nullptr;
    float *dLut = nullptr;
    float *dMid = nullptr, *dBack = nullptr;  // the three-kernel chain's intermediates (236 MB each per 64 frames): made on its first use
    int *dFirstX = nullptr, *dFirstY = nullptr;  // inverse of the stage-A tap tables (fused import, amos_orb.hip)
    bool onePassFits = false;  // the frame size's windows fit k_mask_pre_fused's LDS arrays (the rule stated at the kernel)
    int srcWindowBytes = 0;    // the largest source window of a tile, rows x columns x 3
};

// amos_mask_pre_mode: 1 = one pass where the frame size allows it (default), 0 = always the three kernels; AMOS_MASK_PRE_FUSED=0 / 1 in
// the environment is the initial value, read once.
static int g_pre_fused = -1;  // -1: environment not read yet

static int pre_fused_mode()
{
    if (g_pre_fused < 0) {
        const char *env = getenv("AMOS_MASK_PRE_FUSED");
        g_pre_fused = env && env[0] == '0' ? 0 : 1;
    }
    return g_pre_fused;
}

static int pre_chain_buffers(amos_mask_pre *p)
{
    if (p->dMid && p->dBack) return AMOS_OK;
    AMOS_HIP_CHECK(hipSetDevice(p->device));
    if (!p->dMid) AMOS_HIP_CHECK(hipMalloc((void **)&p->dMid, sizeof(float) * 3 * kMidW * kMidH * (size_t)p->maxBatch));
    if (!p->dBack) AMOS_HIP_CHECK(hipMalloc((void **)&p->dBack, sizeof(float) * 3 * kBackW * kBackH * (size_t)p->maxBatch));
    return AMOS_OK;
}

static void launch_pre_fused(amos_mask_pre *p, hipStream_t stream, const uint8_t *src, size_t frameStride, size_t rowStride, int channels, int n_frames,
                             float *d_out)
{
    const PreTables t{p->dFixX, p->dFixY, p->dFltX, p->dFltY, p->dLut};
    const int tiles = (kNetSize + kPreTile - 1) / kPreTile;
    hipLaunchKernelGGL(k_mask_pre_fused, dim3(tiles, tiles, n_frames), dim3(256), 0, stream, src, frameStride, rowStride, channels, t, d_out);
}

// cv::resize INTER_LINEAR source index and fraction per destination index (double -> float as OpenCV does);
// the horizontal pass clamps the fraction at both ends, the vertical pass only clips the indices.
static void axis_taps(int srcN, int dstN, bool clampFraction, std::vector<int> &s0, std::vector<int> &s1, std::vector<float> &f)
{
    const double scale = 1.0 / ((double)dstN / (double)srcN);
    s0.resize(dstN); s1.resize(dstN); f.resize(dstN);
    for (int d = 0; d < dstN; d++) {
        float fx = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(fx);
        fx -= (float)s;
        if (clampFraction) {
            if (s < 0) { fx = 0; s = 0; }
            if (s >= srcN - 1) { fx = 0; s = srcN - 1; }
        }
        s0[d] = std::min(std::max(s, 0), srcN - 1);
        s1[d] = std::min(std::max(s + 1, 0), srcN - 1);
        f[d] = fx;
    }
}

static int round_even(float v) { return (int)std::nearbyintf(v); }

namespace amos {
int mask_pre_stage_a(amos_mask_pre *p, MaskPreStageA *out, bool withChain)
{
    if (!p || !out) { set_error("mask pre-processing handle missing"); return AMOS_ERR_INVALID; }
    if (withChain) {
        const int rc = pre_chain_buffers(p);
        if (rc != AMOS_OK) return rc;
    }
    *out = MaskPreStageA{p->dFixX, p->dFixY, p->dFirstX, p->dFirstY, p->dLut, p->dMid, p->width, p->height, p->maxBatch};
    return AMOS_OK;
}
bool mask_pre_one_pass(const amos_mask_pre *p) { return p && p->onePassFits && pre_fused_mode() == 1; }
int mask_pre_run_one_pass(amos_mask_pre *p, hipStream_t stream, const uint8_t *d_color, size_t frame_stride, size_t row_stride, int channels, int n_frames,
                          float *d_out)
{
    launch_pre_fused(p, stream, d_color, frame_stride, row_stride, channels, n_frames, d_out);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}
int mask_pre_finish(amos_mask_pre *p, hipStream_t stream, int n_frames, float *d_out)
{
    hipLaunchKernelGGL(k_mask_pre_b, dim3((kBackW * kBackH + 255) / 256, n_frames), dim3(256), 0, stream, p->dMid, p->dFltX, p->dFltY, p->dBack);
    hipLaunchKernelGGL(k_mask_pre_c, dim3((kNetSize * kNetSize + 255) / 256, n_frames), dim3(256), 0, stream, p->dBack, d_out);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}
}  // namespace amos

extern "C" {

int amos_mask_pre_create(int device, void *stream, int width, int height, int max_batch, amos_mask_pre **out)
{
    if (!out || width < 2 || height < 2 || max_batch < 1) { set_error("amos_mask_pre_create: invalid argument"); return AMOS_ERR_INVALID; }
    amos_mask_pre *p = new amos_mask_pre();
    p->width = width; p->height = height; p->maxBatch = max_batch;
    const int rc = p->open(device, stream);
    if (rc != AMOS_OK) { delete p; return rc; }
    std::vector<int> s0, s1;
    std::vector<float> f;
    std::vector<FixTap> hFix[2];  // host copies, x then y: the one-pass kernel's windows are worked out from them below
    std::vector<FltTap> hFlt[2];
    auto fix = [&](int srcN, int dstN, bool clamp, FixTap **dst, int **first) -> hipError_t {
        axis_taps(srcN, dstN, clamp, s0, s1, f);
        std::vector<FixTap> &t = hFix[clamp ? 0 : 1];
        t.resize(dstN);
        for (int d = 0; d < dstN; d++) t[d] = FixTap{s0[d], s1[d], round_even((1.f - f[d]) * 2048.f), round_even(f[d] * 2048.f)};
        // first tap indices are non-decreasing: first[X] = the first destination index whose first tap is >= X
        std::vector<int> inv(srcN + 1);
        for (int X = 0, d = 0; X <= srcN; X++) {
            while (d < dstN && s0[d] < X) d++;
            inv[X] = d;
        }
        hipError_t e = hipMalloc((void **)dst, sizeof(FixTap) * dstN);
        if (e == hipSuccess) e = hipMemcpy(*dst, t.data(), sizeof(FixTap) * dstN, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void **)first, sizeof(int) * inv.size());
        if (e == hipSuccess) e = hipMemcpy(*first, inv.data(), sizeof(int) * inv.size(), hipMemcpyHostToDevice);
        return e;
    };
    auto flt = [&](int srcN, int dstN, bool clamp, FltTap **dst) -> hipError_t {
        axis_taps(srcN, dstN, clamp, s0, s1, f);
        std::vector<FltTap> &t = hFlt[clamp ? 0 : 1];
        t.resize(dstN);
        for (int d = 0; d < dstN; d++) t[d] = FltTap{s0[d], s1[d], 1.0f - f[d], f[d]};
        hipError_t e = hipMalloc((void **)dst, sizeof(FltTap) * dstN);
        if (e != hipSuccess) return e;
        return hipMemcpy(*dst, t.data(), sizeof(FltTap) * dstN, hipMemcpyHostToDevice);
    };
    float lut[256];
    for (int v = 0; v < 256; v++) lut[v] = (float)((double)v / 255.0) * 255.0f;  // yolact.cc:424-431, yolact_interface.py:864
    hipError_t e = fix(width, kMidW, true, &p->dFixX, &p->dFirstX);
    if (e == hipSuccess) e = fix(height, kMidH, false, &p->dFixY, &p->dFirstY);
    if (e == hipSuccess) e = flt(kMidW, kBackW, true, &p->dFltX);
    if (e == hipSuccess) e = flt(kMidH, kBackH, false, &p->dFltY);
    if (e == hipSuccess) e = hipMalloc((void **)&p->dLut, sizeof(lut));
    if (e == hipSuccess) e = hipMemcpy(p->dLut, lut, sizeof(lut), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("amos_mask_pre_create: %s", hipGetErrorString(e));
        amos_mask_pre_destroy(p);
        return AMOS_ERR_DEVICE;
    }
    {   // k_mask_pre_fused's rule for this frame size: tables non-decreasing, every tile's windows inside the LDS arrays
        bool fits = true;
        auto rising = [&](auto &t) {
            for (size_t d = 1; d < t.size(); d++) fits = fits && t[d].s0 >= t[d - 1].s0 && t[d].s1 >= t[d - 1].s1 && t[d].s1 >= t[d].s0;
        };
        rising(hFix[0]); rising(hFix[1]); rising(hFlt[0]); rising(hFlt[1]);
        const float sh = (float)kBackH / (float)kNetSize, sw = (float)kBackW / (float)kNetSize;
        int srcRows = 0, srcCols = 0;
        for (int o0 = 0; fits && o0 < kNetSize; o0 += kPreTile) {
            const int o1 = std::min(o0 + kPreTile, kNetSize) - 1;
            const PreAxisWindow wx = pre_axis_window(o0, o1, kBackW, sw, hFlt[0].data(), hFix[0].data());
            const PreAxisWindow wy = pre_axis_window(o0, o1, kBackH, sh, hFlt[1].data(), hFix[1].data());
            fits = wx.b1 - wx.b0 < kPreBCols && wy.b1 - wy.b0 < kPreBRows && wx.m1 - wx.m0 < kPreACols && wy.m1 - wy.m0 < kPreARows;
            srcCols = std::max(srcCols, wx.s1 - wx.s0 + 1);
            srcRows = std::max(srcRows, wy.s1 - wy.s0 + 1);
        }
        p->srcWindowBytes = srcRows * pre_src_pitch(srcCols);  // (most rows and most columns: an upper bound of every tile's product)
        p->onePassFits = fits && p->srcWindowBytes <= kPreSrcBytes;
    }
    *out = p;
    return AMOS_OK;
}

void amos_mask_pre_destroy(amos_mask_pre *p)
{
    if (!p) return;
    p->close();
    void *ptrs[] = {p->dFixX, p->dFixY, p->dFltX, p->dFltY, p->dLut, p->dMid, p->dBack, p->dFirstX, p->dFirstY};
    for (void *q : ptrs) if (q) (void)hipFree(q);
    delete p;
}

void *amos_mask_pre_stream(amos_mask_pre *p) { return p ? (void *)p->stream : nullptr; }

int amos_mask_pre_mode(int mode)
{
    const int before = pre_fused_mode();
    if (mode == 0 || mode == 1) g_pre_fused = mode;
    return before;
}

int amos_mask_pre_one_pass(const amos_mask_pre *p, int *source_window_bytes)
{
    if (!p) { set_error("amos_mask_pre_one_pass: invalid argument"); return AMOS_ERR_INVALID; }
    if (source_window_bytes) *source_window_bytes = p->srcWindowBytes;
    return mask_pre_one_pass(p) ? 1 : 0;
}

int amos_mask_preprocess_batch_device(amos_mask_pre *p, const uint8_t *d_bgr, int n_frames, float *d_out)
{
    if (!p || !d_bgr || !d_out || n_frames < 1) { set_error("amos_mask_preprocess_batch_device: invalid argument"); return AMOS_ERR_INVALID; }
    if (n_frames > p->maxBatch) { set_error("amos_mask_preprocess_batch_device: %d frames, handle made for %d", n_frames, p->maxBatch); return AMOS_ERR_CAPACITY; }
    AMOS_HIP_CHECK(hipSetDevice(p->device));
    if (mask_pre_one_pass(p))
        return mask_pre_run_one_pass(p, p->stream, d_bgr, (size_t)p->width * p->height * 3, (size_t)p->width * 3, 3, n_frames, d_out);
    const int rc = pre_chain_buffers(p);
    if (rc != AMOS_OK) return rc;
    hipLaunchKernelGGL(k_mask_pre_a, dim3((kMidW * kMidH + 255) / 256, n_frames), dim3(256), 0, p->stream, d_bgr, p->width, p->height, p->dFixX,
                       p->dFixY, p->dLut, p->dMid);
    hipLaunchKernelGGL(k_mask_pre_b, dim3((kBackW * kBackH + 255) / 256, n_frames), dim3(256), 0, p->stream, p->dMid, p->dFltX, p->dFltY, p->dBack);
    hipLaunchKernelGGL(k_mask_pre_c, dim3((kNetSize * kNetSize + 255) / 256, n_frames), dim3(256), 0, p->stream, p->dBack, d_out);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}


int amos_mask_bias_act_device(void *stream, float *d_y, const float *d_bias, const float *d_residual, size_t n, int channels, int relu)
{
    if (!d_y || !d_bias || channels < 1 || n % (size_t)channels != 0) { set_error("amos_mask_bias_act_device: invalid argument"); return AMOS_ERR_INVALID; }
    if (n == 0) return AMOS_OK;
    const bool vec = channels % 4 == 0 && ((uintptr_t)d_y | (uintptr_t)d_bias | (uintptr_t)d_residual) % 16 == 0;
    const dim3 grid((unsigned)((n / 4 + 256) / 256)), block(256);
    const bool pow2 = (channels & (channels - 1)) == 0;
    if (vec && pow2) hipLaunchKernelGGL((k_bias_act<true, true>), grid, block, 0, (hipStream_t)stream, d_y, d_bias, d_residual, n, channels, relu);
    else if (vec) hipLaunchKernelGGL((k_bias_act<true, false>), grid, block, 0, (hipStream_t)stream, d_y, d_bias, d_residual, n, channels, relu);
    else hipLaunchKernelGGL((k_bias_act<false, false>), grid, block, 0, (hipStream_t)stream, d_y, d_bias, d_residual, n, channels, relu);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}


int amos_mask_bias_relu_maxpool_device(void *stream, const float *d_x, const float *d_bias, float *d_y, int n, int in_h, int in_w, int channels)
{
    if (!d_x || !d_bias || !d_y || n < 1 || in_h < 1 || in_w < 1 || channels < 4 || channels % 4 != 0 ||
        ((uintptr_t)d_x | (uintptr_t)d_y | (uintptr_t)d_bias) % 16 != 0 || n > 65535 || in_h > 2 * 65535) {
        set_error("amos_mask_bias_relu_maxpool_device: invalid argument (channels % 4 == 0, 16-byte aligned tensors)");
        return AMOS_ERR_INVALID;
    }
    const int oh = (in_h + 2 - 3) / 2 + 1, ow = (in_w + 2 - 3) / 2 + 1, c4 = channels / 4;
    hipLaunchKernelGGL(k_bias_relu_maxpool, dim3((ow * c4 + 255) / 256, oh, n), dim3(256), 0, (hipStream_t)stream, d_x, d_bias, d_y, in_h, in_w, oh, ow, c4);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}


static std::atomic<int> g_bilinear_x2{1};
int amos_mask_bilinear_x2_mode(int mode)
{
    const int before = g_bilinear_x2.load();
    if (mode == 0 || mode == 1) g_bilinear_x2.store(mode);
    return before;
}

int amos_mask_bilinear_nhwc_act_device(void *stream, const float *d_x, float *d_y, int n, int in_h, int in_w, int out_h, int out_w, int channels,
                                       float scale_h, float scale_w, int relu)
{
    if (!d_x || !d_y || n < 1 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || channels < 4 || channels % 4 != 0 ||
        ((uintptr_t)d_x | (uintptr_t)d_y) % 16 != 0 || out_h > 65535 || n > 65535) {
        set_error("amos_mask_bilinear_nhwc_device: invalid argument (channels % 4 == 0, 16-byte aligned tensors)");
        return AMOS_ERR_INVALID;
    }
    const int c4 = channels / 4;
    if (g_bilinear_x2 && out_h == 2 * in_h && out_w == 2 * in_w && scale_h == 0.5f && scale_w == 0.5f) {  // an exact x 2 enlargement: 2 x 2 outputs per thread
        const dim3 grid2((unsigned)(((long long)((out_h + 1) / 2) * ((out_w + 1) / 2) * c4 + 255) / 256), 1, n);
        if (relu) hipLaunchKernelGGL(k_bilinear_nhwc_x2<true>, grid2, dim3(256), 0, (hipStream_t)stream, d_x, d_y, in_h, in_w, out_h, out_w, c4, scale_h, scale_w);
        else hipLaunchKernelGGL(k_bilinear_nhwc_x2<false>, grid2, dim3(256), 0, (hipStream_t)stream, d_x, d_y, in_h, in_w, out_h, out_w, c4, scale_h, scale_w);
        AMOS_HIP_CHECK(hipGetLastError());
        return AMOS_OK;
    }
    const dim3 grid((out_w * c4 + 255) / 256, out_h, n), block(256);
    if (relu) hipLaunchKernelGGL(k_bilinear_nhwc<true>, grid, block, 0, (hipStream_t)stream, d_x, d_y, in_h, in_w, out_h, out_w, c4, scale_h, scale_w);
    else hipLaunchKernelGGL(k_bilinear_nhwc<false>, grid, block, 0, (hipStream_t)stream, d_x, d_y, in_h, in_w, out_h, out_w, c4, scale_h, scale_w);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

int amos_mask_bilinear_nhwc_device(void *stream, const float *d_x, float *d_y, int n, int in_h, int in_w, int out_h, int out_w, int channels,
                                   float scale_h, float scale_w)
{
    return amos_mask_bilinear_nhwc_act_device(stream, d_x, d_y, n, in_h, in_w, out_h, out_w, channels, scale_h, scale_w, 0);
}

int amos_mask_nms_column_max_device(void *stream, const float *d_boxes, float *d_out, int n_lists, int k)
{
    if (!d_boxes || !d_out || n_lists < 0 || k < 1 || k > 256 || (uintptr_t)d_boxes % 16 != 0) {
        set_error("amos_mask_nms_column_max_device: invalid argument (1 <= k <= 256, 16-byte aligned boxes)");
        return AMOS_ERR_INVALID;
    }
    if (n_lists == 0) return AMOS_OK;
    hipLaunchKernelGGL(k_nms_column_max, dim3(n_lists), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(d_boxes), d_out, k);
    AMOS_HIP_CHECK(hipGetLastError());
    return AMOS_OK;
}

}  // extern "C"
