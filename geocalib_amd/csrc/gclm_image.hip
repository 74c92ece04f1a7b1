// gclm_image.hip -- gclm_undistort_image: BaseCamera.undistort_image (reference geocalib/camera.py:396-412) in one pass.
//
// The reference builds a (1, H, W, 2) sampling grid from ten torch ops (meshgrid, normalize, Pinhole.undistort, the
// projection of (u, v, 1), the model's distort, denormalize, the align_corners normalisation) and resamples with
// F.grid_sample(bilinear, zeros, align_corners=True).  Here each lane computes its output pixel's source coordinate in
// registers, once for all channels, and loops over the channels with the four taps' offsets and weights held:
//   u = (x - cx) / fx,  v = (y - cy) / fy,  r2 = u^2 + v^2,  s = s_model(r2)
//   ix = ((x - cx) s + cx) (Win - 1) / (W - 1),   iy = ((y - cy) s + cy) (Hin - 1) / (H - 1)
// which is the reference's denormalize(distort(normalize(x))) followed by grid_sample's unnormalisation, in exact
// arithmetic.  Integer pixel centres, no half-pixel offset (as the reference's meshgrid).  With s = 1, c exactly
// representable and Win = W the output is a bit-exact copy of the input.
//
// simple_divisional: s = (1 - sqrt(1 - 4 k r2)) / (2 k r2) cancels in float32 (1.3 % off at |k r2| = 1e-6, 13 px at 1000 px
// from the centre).  The identical s = 2 / (1 + sqrt(t)), t = 1 - 4 k r2 > 0, does not; where t <= 0 the clamp of the
// reference leaves s = 1 / (2 k r2).  The LM sweep (gclm_pass.hip) keeps the cancelling form on purpose, to match the
// reference's float32 rounding inside the solve; a resampler has no such reason and is held to float64.
//
// Zero padding as grid_sample's: each tap contributes only if it lies in [0, Win) x [0, Hin), and is not read otherwise.
// A non-finite coordinate (NaN or inf camera, or an overflow) contributes nothing: the output pixel is 0.
//
// Layout: one wave walks 64 adjacent output pixels of a row (GCLM_UNDIST_PX = 2: 128, two per lane, dwordx2 stores), a
// block of 4 waves covers 4 rows, grid = (tiles of one image, B).  No LDS, no scratch, no barrier.
#include "gclm_internal.h"

// Measured variants (DESIGN.md 3.5, 1920x1080, C = 3, B = 1 / 16 / 64): nontemporal stores -3 ... -13 % kernel time, kept;
// two pixels per lane +23 ... +52 %, the XCD-banded block order +5 ... +11 %, both off.
#ifndef GCLM_UNDIST_PX
#define GCLM_UNDIST_PX 1        // output pixels per lane (2: dwordx2 stores, used when W is even)
#endif
#ifndef GCLM_UNDIST_NT
#define GCLM_UNDIST_NT 1        // 1: nontemporal stores to the destination (0: plain stores)
#endif
#ifndef GCLM_UNDIST_XCD
#define GCLM_UNDIST_XCD 0       // 1: remap blocks so that each XCD walks one contiguous band of tiles of an image
#endif

namespace gclm {
namespace {

constexpr int kRows = 4;        // rows per block: one per wave
typedef float f32x2 __attribute__((ext_vector_type(2)));     // (HIP's float2 is a struct: no nontemporal store)

template <int MODEL>
__device__ __forceinline__ float undistort_distort_scale(float r2, float k1, float k2) {
    if constexpr (MODEL == GCLM_PINHOLE) {
        return 1.f;
    } else if constexpr (MODEL == GCLM_SIMPLE_RADIAL) {
        return 1.f + k1 * r2;
    } else if constexpr (MODEL == GCLM_RADIAL) {
        return 1.f + (k1 + k2 * r2) * r2;
    } else {
        const float kr = k1 * r2, t = 1.f - 4.f * kr;
        if (kr == 0.f) return 1.f;
        return t > 0.f ? 2.f / (1.f + sqrtf(t)) : 1.f / (2.f * kr);
    }
}

// One output pixel's taps: 64-bit offset of the top-left tap, bilinear weights, which taps lie inside the source.
struct Taps {
    int64_t o;
    float w00, w01, w10, w11;
    bool m00, m01, m10, m11;
};

template <int MODEL>
__device__ __forceinline__ Taps undistort_taps(int x, int y, float ifx, float ify, float cx, float cy, float k1, float k2,
                                               float sx, float sy, int Hin, int Win) {
    const float dx = (float)x - cx, dy = (float)y - cy;
    const float u = dx * ifx, v = dy * ify;
    const float s = undistort_distort_scale<MODEL>(u * u + v * v, k1, k2);
    float ix = (dx * s + cx) * sx, iy = (dy * s + cy) * sy;
    // NaN -> -2, +-inf and overflows -> just outside the source: every tap then lies outside and the pixel is 0
    ix = ix == ix ? fminf(fmaxf(ix, -2.f), (float)Win + 1.f) : -2.f;
    iy = iy == iy ? fminf(fmaxf(iy, -2.f), (float)Hin + 1.f) : -2.f;
    const float x0 = floorf(ix), y0 = floorf(iy);
    const int xi = (int)x0, yi = (int)y0;
    const float ax = ix - x0, ay = iy - y0, bx = 1.f - ax, by = 1.f - ay;
    const bool mx0 = (unsigned)xi < (unsigned)Win, mx1 = (unsigned)(xi + 1) < (unsigned)Win;
    const bool my0 = (unsigned)yi < (unsigned)Hin, my1 = (unsigned)(yi + 1) < (unsigned)Hin;
    Taps t;
    t.o = (int64_t)yi * Win + xi;
    t.w00 = bx * by; t.w01 = ax * by; t.w10 = bx * ay; t.w11 = ax * ay;     // grid_sample's nw, ne, sw, se
    t.m00 = mx0 && my0; t.m01 = mx1 && my0; t.m10 = mx0 && my1; t.m11 = mx1 && my1;
    return t;
}

__device__ __forceinline__ float undistort_sample(const float* __restrict__ p, const Taps& t, int Win) {
    const float v00 = t.m00 ? p[t.o] : 0.f, v01 = t.m01 ? p[t.o + 1] : 0.f;
    const float v10 = t.m10 ? p[t.o + Win] : 0.f, v11 = t.m11 ? p[t.o + Win + 1] : 0.f;
    return v00 * t.w00 + v01 * t.w01 + v10 * t.w10 + v11 * t.w11;
}

template <bool NT, typename T>
__device__ __forceinline__ void undistort_store(T v, T* p) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <int MODEL, int PX, bool NT, bool XCD>
__global__ __launch_bounds__(kBlock) void undistort_image_kernel(const float* __restrict__ cam, int cam_stride,
                                                                 const float* __restrict__ src, int C, int Hin, int Win,
                                                                 int H, int W, int tiles_x, int tiles, float* __restrict__ dst) {
    int t = blockIdx.x;
    if constexpr (XCD) {
        // blocks are dealt round-robin over the 8 XCDs (b and b + 8 share one), and gridDim.x is a multiple of 8 here, so
        // blockIdx.x & 7 names the XCD: give XCD j the contiguous band [j q, (j + 1) q) of this image's tiles
        const int q = gridDim.x >> 3;
        t = (t & 7) * q + (t >> 3);
    }
    if (t >= tiles) return;
    const int b = blockIdx.y;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y = ty * kRows + (threadIdx.x >> 6);
    const int x = (tx * 64 + (threadIdx.x & 63)) * PX;
    if (y >= H || x >= W) return;
    const float* cb = cam + (size_t)b * cam_stride;
    const float fx = cb[2], fy = cb[3], cx = cb[4], cy = cb[5], k1 = cb[6], k2 = cb[7];
    const float ifx = 1.f / fx, ify = 1.f / fy;
    const float sx = (float)(Win - 1) / (float)(W - 1), sy = (float)(Hin - 1) / (float)(H - 1);
    const size_t plane_in = (size_t)Hin * Win, plane_out = (size_t)H * W;
    const float* s = src + (size_t)b * C * plane_in;
    float* d = dst + (size_t)b * C * plane_out + (size_t)y * W + x;
    if constexpr (PX == 1) {
        const Taps a = undistort_taps<MODEL>(x, y, ifx, ify, cx, cy, k1, k2, sx, sy, Hin, Win);
        for (int c = 0; c < C; ++c, s += plane_in, d += plane_out) undistort_store<NT>(undistort_sample(s, a, Win), d);
    } else {
        // PX = 2 runs only for even W: x is even, so x + 1 < W and the float2 store is 8-byte aligned
        const Taps a = undistort_taps<MODEL>(x, y, ifx, ify, cx, cy, k1, k2, sx, sy, Hin, Win);
        const Taps e = undistort_taps<MODEL>(x + 1, y, ifx, ify, cx, cy, k1, k2, sx, sy, Hin, Win);
        for (int c = 0; c < C; ++c, s += plane_in, d += plane_out)
            undistort_store<NT>(f32x2{undistort_sample(s, a, Win), undistort_sample(s, e, Win)}, reinterpret_cast<f32x2*>(d));
    }
}

template <int MODEL, int PX>
hipError_t launch_undistort_px(const float* cam, int cam_batch, const float* src, int B, int C, int Hin, int Win, int H, int W,
                               float* dst, hipStream_t st) {
    const int tiles_x = (W + 64 * PX - 1) / (64 * PX), tiles = tiles_x * ((H + kRows - 1) / kRows);
    const int grid_x = GCLM_UNDIST_XCD ? (tiles + 7) / 8 * 8 : tiles;
    hipLaunchKernelGGL((undistort_image_kernel<MODEL, PX, GCLM_UNDIST_NT != 0, GCLM_UNDIST_XCD != 0>), dim3(grid_x, B),
                       dim3(kBlock), 0, st, cam, cam_batch == 1 ? 0 : 8, src, C, Hin, Win, H, W, tiles_x, tiles, dst);
    return hipGetLastError();
}

template <int MODEL>
hipError_t launch_undistort_model(const float* cam, int cam_batch, const float* src, int B, int C, int Hin, int Win, int H, int W,
                                  float* dst, hipStream_t st) {
    if constexpr (GCLM_UNDIST_PX == 2)
        if (W % 2 == 0) return launch_undistort_px<MODEL, 2>(cam, cam_batch, src, B, C, Hin, Win, H, W, dst, st);
    return launch_undistort_px<MODEL, 1>(cam, cam_batch, src, B, C, Hin, Win, H, W, dst, st);
}

}  // namespace

hipError_t launch_undistort_image(int camera_model, const float* cam, int cam_batch, const float* src, int B, int C, int Hin,
                                  int Win, int H, int W, float* dst, hipStream_t st) {
    switch (camera_model) {
        case GCLM_PINHOLE: return launch_undistort_model<GCLM_PINHOLE>(cam, cam_batch, src, B, C, Hin, Win, H, W, dst, st);
        case GCLM_SIMPLE_RADIAL: return launch_undistort_model<GCLM_SIMPLE_RADIAL>(cam, cam_batch, src, B, C, Hin, Win, H, W, dst, st);
        case GCLM_RADIAL: return launch_undistort_model<GCLM_RADIAL>(cam, cam_batch, src, B, C, Hin, Win, H, W, dst, st);
        case GCLM_SIMPLE_DIVISIONAL:
            return launch_undistort_model<GCLM_SIMPLE_DIVISIONAL>(cam, cam_batch, src, B, C, Hin, Win, H, W, dst, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace gclm
