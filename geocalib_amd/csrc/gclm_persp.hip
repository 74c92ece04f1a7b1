// gclm_persp.hip -- gclm_perspective_fields: get_up_field / get_latitude_field / get_perspective_field (reference
// geocalib/perspective_fields.py:47-74, 185-211, 278-320) in one pass that writes both fields.
//
// The torch composition makes about thirty launches over (B, h w, k) tensors (pixel grid, normalize, the distort scale,
// up_projection_offset, products, F.normalize; image2world, pixel_bearing_many, a dot product, clamp, asin) and walks the
// pixels twice.  Here a lane reads one camera {w, h, fx, fy, cx, cy, k1, k2} and one gravity (a, b, c) per image, computes
// its pixel's fields in registers and only writes:
//   u = (x - cx) / fx,  v = (y - cy) / fy,  r2 = u^2 + v^2            (integer pixel centres, no half-pixel offset)
//   up:  p = (a - c u, b - c v),  q = s(r2) p + 2 s'(r2) (u, v) (u p_x + v p_y)   (pinhole: q = p)
//        normalize: up = q / max(|q|, 1e-12)  (F.normalize);  otherwise up = q
//   lat: t = t(r2),  ray = (u t, v t, 1) / |(u t, v t, 1)|,  lat = asin(clamp(ray . g, -1 + 1e-6, 1 - 1e-6))
// Gravity is used as stored (not renormalised), as the reference's dot product does.  |(u t, v t, 1)| >= 1 or NaN, so the
// reference's max(|.|, 1e-12) guard of the ray never acts and is not evaluated.
//
// s, s' (distort scale and ds/dr2) and t (undistort scale) per model, as camera.py's _distort_scale, _distort_scale_dr2 and
// _undistort_scale: simple_radial s = 1 + k1 r2, s' = k1, t = 1 - k1 r2; radial s = 1 + k1 r2 + k2 r2^2, s' = k1 + 2 k2 r2,
// t = 1 - k1 r2 + (3 k1^2 - k2) r2^2; simple_divisional t = 1 / (1 + k1 r2) (a zero denominator replaced by 1e6) and, with
// tau = 1 - 4 k1 r2, s = 2 / (1 + sqrt(tau)) (tau > 0), 1 / (2 k1 r2) (tau <= 0), 1 (k1 r2 = 0); s' = 4 k1 / (sqrt(tau)
// (1 + sqrt(tau))^2) (tau >= 1e-6), the reference's expression with sqrt(tau) clamped at 1e-3 (tau < 1e-6), 0 (k1 r2 = 0).
// Those are the reference's definitions; its float32 evaluation of s and s' (1 - sqrt(1 - 4 k1 r2) over 2 k1 r2) cancels
// (s 1.3 % off at |k1 r2| = 1e-6), the forms above do not.  The LM sweep keeps the cancelling form on purpose, to match the
// reference's rounding inside the solve; a renderer has no such reason and is held to float64 (tests/perspective_gate.py).
//
// NaN: a NaN or inf in the camera or gravity gives NaN wherever the torch composition gives NaN.  Both guards (the norm's
// 1e-12 floor and the clamp) are comparisons that keep a NaN operand, not fminf / fmaxf, which would drop it.
//
// Layout: up (B, H, W, 2) interleaved, lat (B, H, W, 1); either may be NULL.  One wave walks 128 adjacent pixels of a row
// (64 where W is odd), a block of 4 waves covers 4 rows, grid = (tiles of one image, B).  64-bit offsets.  No LDS, no scratch, no barrier.
#include "gclm_internal.h"

// Measured variants (DESIGN.md 3.7, 640x480, B = 1024, against one pixel per lane with plain stores): two pixels per lane
// -16 % (pinhole) / -8 % (simple_divisional) kernel time, with nontemporal stores on top -22 % / -10 %: both kept.
#ifndef GCLM_PERSP_PX
#define GCLM_PERSP_PX 2         // pixels per lane (2: dwordx4 / dwordx2 stores, used when W is even and the outputs aligned)
#endif
#ifndef GCLM_PERSP_NT
#define GCLM_PERSP_NT 1         // 1: nontemporal stores of both fields (0: plain stores)
#endif

namespace gclm {
namespace {

constexpr int kRows = 4;        // rows per block: one per wave
typedef float f32x2 __attribute__((ext_vector_type(2)));     // (HIP's float2 is a struct: no nontemporal store)
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float kLatHi = (float)(1.0 - 1e-6);                 // the reference's clamp bound, as torch rounds it to float32

template <int MODEL>
__device__ __forceinline__ void persp_distort(float r2, float k1, float k2, float& s, float& sp) {
    if constexpr (MODEL == GCLM_SIMPLE_RADIAL) {
        s = 1.f + k1 * r2;
        sp = k1;
    } else if constexpr (MODEL == GCLM_RADIAL) {
        s = 1.f + (k1 + k2 * r2) * r2;
        sp = k1 + 2.f * k2 * r2;
    } else {
        const float kr = k1 * r2, tau = 1.f - 4.f * kr;
        const float rt = sqrtf(tau > 0.f ? tau : 0.f), d = 1.f + rt;
        s = tau > 0.f ? 2.f / d : 1.f / (2.f * kr);
        if (tau >= 1e-6f) {
            sp = 4.f * k1 / (rt * d * d);
        } else {                // the reference's expression at its clamp sqrt(max(tau, 1e-6)): no cancellation here
            const float tt = sqrtf(1e-6f), den = 2.f * k1 * (r2 * r2) * tt;
            sp = (2.f * k1 * r2 - (1.f - tt) * tt) / (den == 0.f ? 1e6f : den);
        }
        if (kr == 0.f) s = 1.f, sp = 0.f;
    }
}

template <int MODEL>
__device__ __forceinline__ float persp_undistort(float r2, float k1, float k2) {
    if constexpr (MODEL == GCLM_PINHOLE) {
        return 1.f;
    } else if constexpr (MODEL == GCLM_SIMPLE_RADIAL) {
        return 1.f - k1 * r2;
    } else if constexpr (MODEL == GCLM_RADIAL) {
        return 1.f - k1 * r2 + (3.f * k1 * k1 - k2) * (r2 * r2);
    } else {
        const float den = 1.f + k1 * r2;
        return 1.f / (den == 0.f ? 1e6f : den);
    }
}

// Per-image and per-row terms of one lane's pixels.
struct PerspRow {
    float ifx, cx, k1, k2, a, b, c;
    float v, v2, py;            // per row: v, v^2, b - c v
};

template <int MODEL>
__device__ __forceinline__ f32x2 persp_up(const PerspRow& r, float u, float r2, bool normalize) {
    const float px = r.a - r.c * u;
    float qx = px, qy = r.py;
    if constexpr (MODEL != GCLM_PINHOLE) {
        float s, sp;
        persp_distort<MODEL>(r2, r.k1, r.k2, s, sp);
        const float o = 2.f * sp * (u * px + r.v * r.py);
        qx = s * px + o * u;
        qy = s * r.py + o * r.v;
    }
    if (normalize) {
        float n = sqrtf(qx * qx + qy * qy);
        n = n < 1e-12f ? 1e-12f : n;            // F.normalize's clamp_min; a NaN norm stays NaN
        const float in = 1.f / n;
        qx *= in, qy *= in;
    }
    return f32x2{qx, qy};
}

template <int MODEL>
__device__ __forceinline__ float persp_lat(const PerspRow& r, float u, float r2) {
    const float t = persp_undistort<MODEL>(r2, r.k1, r.k2);
    const float X = u * t, Y = r.v * t;
    float sl = (X * r.a + Y * r.b + r.c) / sqrtf(X * X + Y * Y + 1.f);
    sl = sl < -kLatHi ? -kLatHi : (sl > kLatHi ? kLatHi : sl);    // a NaN stays NaN
    return asinf(sl);
}

template <bool NT, typename T>
__device__ __forceinline__ void persp_put(T v, T* p) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <int MODEL, int PX, bool NT>
__global__ __launch_bounds__(kBlock) void perspective_field_kernel(const float* __restrict__ cam, const float* __restrict__ grav,
                                                                   int H, int W, int tiles_x, int normalize,
                                                                   float* __restrict__ up, float* __restrict__ lat) {
    const int b = blockIdx.y, t = blockIdx.x;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y = ty * kRows + (threadIdx.x >> 6);
    const int x = (tx * 64 + (threadIdx.x & 63)) * PX;
    if (y >= H || x >= W) return;
    const float* cb = cam + (size_t)b * 8;
    const float* gb = grav + (size_t)b * 3;
    PerspRow r;
    r.ifx = 1.f / cb[2];
    r.cx = cb[4], r.k1 = cb[6], r.k2 = cb[7];
    r.a = gb[0], r.b = gb[1], r.c = gb[2];
    r.v = ((float)y - cb[5]) * (1.f / cb[3]);
    r.v2 = r.v * r.v;
    r.py = r.b - r.c * r.v;
    const size_t o = ((size_t)b * H + y) * W + x;
    const bool nrm = normalize != 0;
    if constexpr (PX == 1) {
        const float u = ((float)x - r.cx) * r.ifx, r2 = u * u + r.v2;
        if (up) persp_put<NT>(persp_up<MODEL>(r, u, r2, nrm), reinterpret_cast<f32x2*>(up + 2 * o));
        if (lat) persp_put<NT>(persp_lat<MODEL>(r, u, r2), lat + o);
    } else {
        // PX = 2 runs only for even W with 16-byte aligned up and 8-byte aligned lat: x is even, so x + 1 < W and o is even
        const float u0 = ((float)x - r.cx) * r.ifx, u1 = ((float)(x + 1) - r.cx) * r.ifx;
        const float r20 = u0 * u0 + r.v2, r21 = u1 * u1 + r.v2;
        if (up) {
            const f32x2 e = persp_up<MODEL>(r, u0, r20, nrm), f = persp_up<MODEL>(r, u1, r21, nrm);
            persp_put<NT>(f32x4{e.x, e.y, f.x, f.y}, reinterpret_cast<f32x4*>(up + 2 * o));
        }
        if (lat) persp_put<NT>(f32x2{persp_lat<MODEL>(r, u0, r20), persp_lat<MODEL>(r, u1, r21)}, reinterpret_cast<f32x2*>(lat + o));
    }
}

template <int MODEL, int PX>
hipError_t launch_persp_px(const float* cam, const float* grav, int B, int H, int W, int normalize, float* up, float* lat,
                           hipStream_t st) {
    const int tiles_x = (W + 64 * PX - 1) / (64 * PX), tiles = tiles_x * ((H + kRows - 1) / kRows);
    hipLaunchKernelGGL((perspective_field_kernel<MODEL, PX, GCLM_PERSP_NT != 0>), dim3(tiles, B), dim3(kBlock), 0, st, cam,
                       grav, H, W, tiles_x, normalize, up, lat);
    return hipGetLastError();
}

template <int MODEL>
hipError_t launch_persp_model(const float* cam, const float* grav, int B, int H, int W, int normalize, float* up, float* lat,
                              hipStream_t st) {
    if constexpr (GCLM_PERSP_PX == 2)
        if (W % 2 == 0 && reinterpret_cast<uintptr_t>(up) % 16 == 0 && reinterpret_cast<uintptr_t>(lat) % 8 == 0)
            return launch_persp_px<MODEL, 2>(cam, grav, B, H, W, normalize, up, lat, st);
    return launch_persp_px<MODEL, 1>(cam, grav, B, H, W, normalize, up, lat, st);
}

}  // namespace

hipError_t launch_perspective_fields(int camera_model, const float* cam, const float* grav, int B, int H, int W, int normalize,
                                     float* up, float* lat, hipStream_t st) {
    switch (camera_model) {
        case GCLM_PINHOLE: return launch_persp_model<GCLM_PINHOLE>(cam, grav, B, H, W, normalize, up, lat, st);
        case GCLM_SIMPLE_RADIAL: return launch_persp_model<GCLM_SIMPLE_RADIAL>(cam, grav, B, H, W, normalize, up, lat, st);
        case GCLM_RADIAL: return launch_persp_model<GCLM_RADIAL>(cam, grav, B, H, W, normalize, up, lat, st);
        case GCLM_SIMPLE_DIVISIONAL: return launch_persp_model<GCLM_SIMPLE_DIVISIONAL>(cam, grav, B, H, W, normalize, up, lat, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace gclm
