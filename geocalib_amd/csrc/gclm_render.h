// gclm_render.h -- the per-pixel core of the one-pass kernels over the tile geometry below.  Included by twelve kernel files --
// the renderers gclm_image.hip, gclm_pano.hip, gclm_reproject.hip, gclm_persp.hip and gclm_overlay.hip, and the kernels that
// score, fit or differentiate predicted fields, gclm_metrics.hip, gclm_hypotheses.hip, gclm_param_opt.hip,
// gclm_field_loss.hip, gclm_bin_loss.hip, gclm_field_param_grad.hip and gclm_lm_grad.hip -- and by gclm_entry.hip, for the bound on the tile grid: the camera models'
// undistort and distort scales, the zero-padded bilinear sampler (float32 images, and uint8 images planar or interleaved
// with their rounding store), the nontemporal store, the tile geometry, the perspective fields of one pixel, and the tile
// walk of the second group ("The tile walk" below: pixels per lane, per-row terms, wave sum, tile record, chain sum).
// Each kernel keeps its own coordinate formula, argument struct, record layout and finish epilogue.
//
// Nothing here is shared with the LM sweep (gclm_pass.hip) or with synth_kernel (gclm_synth.hip), on purpose: the sweep
// keeps the reference's float32 forms so that the solve rounds like the reference, and the synthetic fields' bits define
// the benchmark's inputs.
#pragma once
#include <initializer_list>

#include "gclm_internal.h"

namespace gclm {

typedef float f32x2 __attribute__((ext_vector_type(2)));     // (HIP's float2 / float4 are structs: no nontemporal store)
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Tile geometry: one wave walks 64 PX adjacent output pixels of a row (PX pixels per lane), a block of 4 waves covers 4 rows,
// grid = (tiles of one image, images).  No LDS, no barrier.
constexpr int kTileRows = kBlock / 64;                        // rows per block: one per wave
constexpr int tile_columns(int W, int px = 1) { return (W + 64 * px - 1) / (64 * px); }
constexpr int tile_count(int H, int W, int px = 1) { return tile_columns(W, px) * ((H + kTileRows - 1) / kTileRows); }
// The largest image of a call (host): its pixels are counted in an int, the threads of its widest grid (px = 1) in 32 bits.
constexpr bool tile_grid_fits(int H, int W) {
    return (int64_t)H * W <= INT32_MAX && (((int64_t)W + 63) / 64) * (((int64_t)H + kTileRows - 1) / kTileRows) * kBlock <= UINT32_MAX;
}

// This lane's first pixel (x, y); false where it lies outside the image.
template <int PX = 1>
__device__ __forceinline__ bool tile_pixel(int tiles_x, int H, int W, int& x, int& y) {
    const int t = blockIdx.x, ty = t / tiles_x, tx = t - ty * tiles_x;
    y = ty * kTileRows + (threadIdx.x >> 6);
    x = (tx * 64 + (threadIdx.x & 63)) * PX;
    return y < H && x < W;
}

// Nontemporal stores of the outputs, which the kernels never read back (measured against plain stores).
template <typename T>
__device__ __forceinline__ void store_nt(T v, T* p) {
    __builtin_nontemporal_store(v, p);
}

// t(r2), the undistort scale of image2world (camera.py's _undistort_scale): pinhole 1; simple_radial 1 - k1 r2; radial
// 1 - k1 r2 + (3 k1^2 - k2) r2^2; simple_divisional 1 / (1 + k1 r2), a zero denominator replaced by 1e6 (the reference's
// masked_fill).
template <int MODEL>
__device__ __forceinline__ float undistort_scale(float r2, float k1, float k2) {
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

// s(r2) and s' = ds/dr2, the distort scale (camera.py's _distort_scale, _distort_scale_dr2): pinhole s = 1, s' = 0;
// simple_radial s = 1 + k1 r2, s' = k1; radial s = 1 + k1 r2 + k2 r2^2, s' = k1 + 2 k2 r2; simple_divisional, with
// tau = 1 - 4 k1 r2, s = 2 / (1 + sqrt(tau)) (tau > 0), 1 / (2 k1 r2) (tau <= 0: what the reference's clamp leaves),
// 1 (k1 r2 = 0); s' = 4 k1 / (sqrt(tau) (1 + sqrt(tau))^2) (tau >= 1e-6), the reference's expression with sqrt(tau) clamped
// at 1e-3 (tau < 1e-6), 0 (k1 r2 = 0).  A caller that needs s alone ignores s'.
// Those are the reference's definitions; its float32 evaluation, (1 - sqrt(1 - 4 k1 r2)) / (2 k1 r2), cancels (s 1.3 % off
// at |k1 r2| = 1e-6, 13 px at 1000 px from the centre), the forms above do not.  The LM sweep (gclm_pass.hip) keeps the
// cancelling form on purpose, to match the reference's float32 rounding inside the solve; a renderer has no such reason
// and is held to float64 (tests/undistort_gate.py, tests/perspective_gate.py).
template <int MODEL>
__device__ __forceinline__ void distort_scale(float r2, float k1, float k2, float& s, float& sp) {
    if constexpr (MODEL == GCLM_PINHOLE) {
        s = 1.f;
        sp = 0.f;
    } else if constexpr (MODEL == GCLM_SIMPLE_RADIAL) {
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

// Bilinear sampling with zero padding, as F.grid_sample(bilinear, zeros, align_corners=True): each tap contributes only if
// it lies in [0, Win) x [0, Hin), and is not read otherwise.  A non-finite coordinate contributes nothing: the sample is 0.
// One pixel's taps: 64-bit offset of the top-left tap, bilinear weights, which taps lie inside the source.
struct Taps {
    int64_t o;
    float w00, w01, w10, w11;
    bool m00, m01, m10, m11;
};

__device__ __forceinline__ Taps bilinear_taps(float ix, float iy, int Hin, int Win) {
    // NaN -> -2, +-inf and overflows -> just outside the source: every tap then lies outside and the sample is 0
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

// One channel's sample: p is the channel's plane, Win its row stride.
__device__ __forceinline__ float bilinear_sample(const float* __restrict__ p, const Taps& t, int Win) {
    const float v00 = t.m00 ? p[t.o] : 0.f, v01 = t.m01 ? p[t.o + 1] : 0.f;
    const float v10 = t.m10 ? p[t.o + Win] : 0.f, v11 = t.m11 ? p[t.o + Win + 1] : 0.f;
    return v00 * t.w00 + v01 * t.w01 + v10 * t.w10 + v11 * t.w11;
}

// Byte images (gclm_undistort_image_u8, gclm_reproject_image_u8: the unsigned char instantiations of undistort_image_kernel and
// reproject_kernel, whose tail is sample_store_u8).  A tap's byte is converted to float32
// exactly, the sample is the float sampler's sum, and the byte written is that sum rounded to nearest, ties to even, saturated
// to 0..255 (the sum of four weighted bytes is finite, so the clamp sees no NaN).
__device__ __forceinline__ unsigned char to_u8(float v) {
    return (unsigned char)(int)fminf(fmaxf(__builtin_rintf(v), 0.f), 255.f);
}

// One channel's sample of a byte image: p + o is the top-left tap's byte, dx the bytes to its right neighbour (1 planar, C
// interleaved), dy the bytes to the row below.
__device__ __forceinline__ float bilinear_sample_u8(const unsigned char* __restrict__ p, const Taps& t, int64_t o, int dx, int64_t dy) {
    const float v00 = t.m00 ? (float)p[o] : 0.f, v01 = t.m01 ? (float)p[o + dx] : 0.f;
    const float v10 = t.m10 ? (float)p[o + dy] : 0.f, v11 = t.m11 ? (float)p[o + dy + dx] : 0.f;
    return v00 * t.w00 + v01 * t.w01 + v10 * t.w10 + v11 * t.w11;
}

// All four channels of an interleaved C = 4 pixel whose image starts on a dword: a tap is one dword, the pixel one dword store.
__device__ __forceinline__ unsigned bilinear_sample_4xu8(const unsigned* __restrict__ p, const Taps& t, int Win) {
    const unsigned v00 = t.m00 ? p[t.o] : 0u, v01 = t.m01 ? p[t.o + 1] : 0u;
    const unsigned v10 = t.m10 ? p[t.o + Win] : 0u, v11 = t.m11 ? p[t.o + Win + 1] : 0u;
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const float v = (float)((v00 >> k) & 255u) * t.w00 + (float)((v01 >> k) & 255u) * t.w01 +
                        (float)((v10 >> k) & 255u) * t.w10 + (float)((v11 >> k) & 255u) * t.w11;
        out |= (unsigned)to_u8(v) << k;
    }
    return out;
}

// Every channel of one output pixel of image b, sampled at `a` and stored: o is the pixel's offset in its (H, W) plane.
// Planar: source (B, C, Hin, Win), destination (B, C, H, W).  Interleaved: (B, Hin, Win, C) and (B, H, W, C), C <= 4;
// `dwords` (host: C = 4 and both images on a 4-byte boundary) takes the dword path, which writes the same bytes.
template <bool INTERLEAVED>
__device__ __forceinline__ void sample_store_u8(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, const Taps& a,
                                                int b, int C, int Hin, int Win, size_t plane_out, int o, bool dwords) {
    const size_t plane_in = (size_t)Hin * Win;
    const unsigned char* p = src + (size_t)b * C * plane_in;
    if constexpr (INTERLEAVED) {
        unsigned char* d = dst + ((size_t)b * plane_out + o) * C;
        if (dwords) {
            store_nt(bilinear_sample_4xu8(reinterpret_cast<const unsigned*>(p), a, Win), reinterpret_cast<unsigned*>(d));
            return;
        }
        const int64_t o00 = a.o * C, dy = (int64_t)Win * C;
        for (int c = 0; c < C; ++c) store_nt(to_u8(bilinear_sample_u8(p, a, o00 + c, C, dy)), d + c);
    } else {
        unsigned char* d = dst + (size_t)b * C * plane_out + o;
        for (int c = 0; c < C; ++c, p += plane_in, d += plane_out) store_nt(to_u8(bilinear_sample_u8(p, a, a.o, 1, Win)), d);
    }
}

// The perspective fields of one pixel (gclm_persp.hip renders them, gclm_metrics.hip scores predictions against them; the
// formulas are in gclm_persp.hip's header and include/gclm.h: gclm_perspective_fields).
constexpr float kLatHi = (float)(1.0 - 1e-6);                 // the reference's clamp bound, as torch rounds it to float32

// Per-image and per-row terms of one lane's pixels.
struct PerspRow {
    float ifx, cx, k1, k2, a, b, c;
    float v, v2, py;            // per row: v, v^2, b - c v
};

// The row's terms at normalised height v.
__device__ __forceinline__ void persp_set_row(PerspRow& r, float v) {
    r.v = v;
    r.v2 = r.v * r.v;
    r.py = r.b - r.c * r.v;
}

// The terms of row y of the image with camera row cb = {w, h, fx, fy, cx, cy, k1, k2} and gravity gb = (a, b, c).
__device__ __forceinline__ PerspRow persp_row(const float* cb, const float* gb, int y) {
    PerspRow r;
    r.ifx = 1.f / cb[2];
    r.cx = cb[4], r.k1 = cb[6], r.k2 = cb[7];
    r.a = gb[0], r.b = gb[1], r.c = gb[2];
    persp_set_row(r, ((float)y - cb[5]) * (1.f / cb[3]));
    return r;
}

template <int MODEL>
__device__ __forceinline__ f32x2 persp_up(const PerspRow& r, float u, float r2, bool normalize) {
    const float px = r.a - r.c * u;
    float qx = px, qy = r.py;
    if constexpr (MODEL != GCLM_PINHOLE) {
        float s, sp;
        distort_scale<MODEL>(r2, r.k1, r.k2, s, sp);
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
    const float t = undistort_scale<MODEL>(r2, r.k1, r.k2);
    const float X = u * t, Y = r.v * t;
    float sl = (X * r.a + Y * r.b + r.c) / sqrtf(X * X + Y * Y + 1.f);
    sl = sl < -kLatHi ? -kLatHi : (sl > kLatHi ? kLatHi : sl);    // a NaN stays NaN
    return asinf(sl);
}

// t' = dt/dr2 of undistort_scale (gclm_overlay.hip: the latitude's gradient): pinhole 0; simple_radial -k1; radial
// -k1 + 2 (3 k1^2 - k2) r2; simple_divisional -k1 t^2 with t as undistort_scale gives it.
template <int MODEL>
__device__ __forceinline__ float undistort_scale_dr2(float r2, float k1, float k2) {
    if constexpr (MODEL == GCLM_PINHOLE) {
        return 0.f;
    } else if constexpr (MODEL == GCLM_SIMPLE_RADIAL) {
        return -k1;
    } else if constexpr (MODEL == GCLM_RADIAL) {
        return -k1 + 2.f * (3.f * k1 * k1 - k2) * r2;
    } else {
        const float t = undistort_scale<MODEL>(r2, k1, k2);
        return -k1 * t * t;
    }
}

// Degrees of latitude per pixel at the pixel persp_lat is taken at: |grad_xy s| (180 / pi) / sqrt(1 - s_c^2), with s the sine
// persp_lat takes asin of, s_c its clamped value, and grad s in closed form (include/gclm.h: gclm_draw_fields): grad_P s =
// (g_xy - s P / n) / n for P = (u t, v t), n = |(P, 1)|;  dP/d(u, v) = t I + 2 t' (u, v)(u, v)^T;  d/dx = ifx d/du, d/dy = ify d/dv.
// The first lines repeat persp_lat's, so that a kernel calling both evaluates them once.  A NaN stays NaN.
template <int MODEL>
__device__ __forceinline__ float persp_lat_slope(const PerspRow& r, float u, float r2, float ify) {
    const float t = undistort_scale<MODEL>(r2, r.k1, r.k2), tp = undistort_scale_dr2<MODEL>(r2, r.k1, r.k2);
    const float X = u * t, Y = r.v * t;
    const float n = sqrtf(X * X + Y * Y + 1.f), in = 1.f / n;
    const float sl = (X * r.a + Y * r.b + r.c) / n;
    const float gX = (r.a - sl * X * in) * in, gY = (r.b - sl * Y * in) * in;
    float du = t * gX, dv = t * gY;
    if constexpr (MODEL != GCLM_PINHOLE) {
        const float w = 2.f * tp * (u * gX + r.v * gY);
        du += w * u, dv += w * r.v;
    }
    const float sx = du * r.ifx, sy = dv * ify;
    const float sc = sl < -kLatHi ? -kLatHi : (sl > kLatHi ? kLatHi : sl);
    return sqrtf(sx * sx + sy * sy) * 57.29577951308232f / sqrtf((1.f - sc) * (1.f + sc));
}

// The tile walk of the kernels that reduce an image's pixels to a few numbers per image (gclm_metrics.hip,
// gclm_hypotheses.hip, gclm_param_opt.hip, gclm_field_loss.hip, gclm_bin_loss.hip, gclm_field_param_grad.hip, gclm_lm_grad.hip).  Every rule stands here
// once; each kernel keeps its per-pixel body, its record layout and what its finish kernel makes of the sums.
//   - (gclm_bin_loss.hip walks the same tiles with 8, 4 or 1 pixels per lane by its logits' type, and adds a lane's pixels in
//     the one-pixel walk's tree so that its records do not depend on the width: see its header)
//   - grid = (tiles of one image, .., images) over the tile geometry above, PX = 4, 2 or 1 pixels per lane
//     (pixels_per_lane: by W and the planes' alignment; the planes of every image of a batch share the alignment of the
//     first, so an image's path does not depend on its place in the batch); load_px / store_px move a lane's pixels.
//   - A lane sums its pixels in its own type (float; float64 in gclm_lm_grad.hip and gclm_field_param_grad.hip, which write
//     wave_sum's butterfly out on doubles); a lane outside the image adds zeros.  wave_sum adds the lanes of a wave, lane 0 leaves the wave's record in
//     LDS, and after ONE barrier thread k adds word k of the kTileRows waves in order and stores it (tile_record): one
//     record per tile in the caller's workspace, which is sized for one pixel per lane, the path with the most tiles
//     (tile_record_bytes).
//   - The finish kernel (one block per image) sums word k of the image's records in float64 in CHAINS strided chains
//     (chain_sum: record t goes to chain t % CHAINS) and adds the chains in order (column_sum).
// No atomics, no block waits on another: the bits of an image's sums depend on that image's pixels, H, W, the pixels per
// lane and the kernel's chain count alone.
// Written out where the shared function changed a kernel's instruction stream (profiles/tile_walk_asm_equal.log): the
// float64 butterfly of lm_grad_pixel_kernel, and the chain walk of field_error_finish_kernel over words of two types.

// Pixels per lane of a call (host): 4 (dwordx4) where W % 4 == 0 and every plane is 16-byte aligned, else 2 (dwordx2) where
// W is even and every plane 8-byte aligned, else 1.  A NULL plane is aligned.  PX > 1 thus runs only where W % PX == 0: a
// lane's x is a multiple of PX, so x + PX <= W, and its vector loads and stores are aligned.
inline int pixels_per_lane(int W, std::initializer_list<const void*> planes, int max_px = 4) {
    uintptr_t bits = 0;
    for (const void* p : planes) bits |= reinterpret_cast<uintptr_t>(p);
    if (max_px >= 4 && W % 4 == 0 && bits % 16 == 0) return 4;
    return W % 2 == 0 && bits % 8 == 0 ? 2 : 1;
}

// Where px becomes a template argument, as with_camera_model: returns f(std::integral_constant<int, PX>{}).  Host code.
template <int MAX_PX = 4, typename F>
auto with_pixels_per_lane(int px, F&& f) {
    if constexpr (MAX_PX >= 4) {
        if (px == 4) return f(std::integral_constant<int, 4>{});
    }
    return px == 2 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 1>{});
}

// The sizes every such call takes (host), and the bytes of its tile records: at one pixel per lane, the path with the most tiles.
constexpr bool call_sizes_fit(int B, int H, int W) { return B >= 1 && B <= kMaxCallImages && H >= 1 && W >= 1 && tile_grid_fits(H, W); }
constexpr size_t tile_record_bytes(size_t images, int H, int W, size_t words, size_t bytes_per_word) {
    return images * tile_count(H, W, 1) * words * bytes_per_word;
}

template <int PX>
__device__ __forceinline__ void load_px(const float* __restrict__ p, float (&v)[PX]) {
    if constexpr (PX == 1) {
        v[0] = *p;
    } else if constexpr (PX == 2) {
        const f32x2 t = *reinterpret_cast<const f32x2*>(p);
        v[0] = t.x, v[1] = t.y;
    } else {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    }
}

// ... and stores them: nontemporal (NT) for a plane the caller reads much later, plain for one that is read next.
template <bool NT, typename T>
__device__ __forceinline__ void store_as(T v, T* p) {
    if constexpr (NT) store_nt(v, p);
    else *p = v;
}
template <int PX, bool NT = true>
__device__ __forceinline__ void store_px(const float (&v)[PX], float* p) {
    if constexpr (PX == 1) {
        store_as<NT>(v[0], p);
    } else if constexpr (PX == 2) {
        store_as<NT>(f32x2{v[0], v[1]}, reinterpret_cast<f32x2*>(p));
    } else {
        store_as<NT>(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4*>(p));
    }
}

// Sum over the 64 lanes of a wave, the same bits in every lane (a butterfly: lane i adds lane i ^ o, o = 32 .. 1).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// s[0][k] + s[1][k] + .. in that order: the waves of a tile, or the chains of a finish kernel.
template <typename T, int N, int WORDS>
__device__ __forceinline__ T column_sum(const T (&s)[N][WORDS], int k) {
    T v = s[0][k];
    for (int i = 1; i < N; ++i) v += s[i][k];
    return v;
}

// The tail of a tile: `s` is the kernel's LDS array, `wave` this thread's row of it (threadIdx.x >> 6, which the kernel has
// at hand), `sum` the wave's sums, the same in every lane; store(k, v) writes word k of the tile's record (thread k calls
// it, so the record's address is formed by that thread alone).  Every thread of the block calls tile_record.
template <typename T, int WORDS, typename Store>
__device__ __forceinline__ void tile_record(T (&s)[kTileRows][WORDS], int wave, const T (&sum)[WORDS], Store&& store) {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) s[wave][k] = sum[k];
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < WORDS) store(k, column_sum(s, k));
}

// Chain `chain` of CHAINS over the records p[0], p[stride], .. of `tiles` tiles: WORDS adjacent words each, in float64.
template <int CHAINS, int WORDS, typename T>
__device__ __forceinline__ void chain_sum(const T* p, size_t stride, int tiles, int chain, double (&acc)[WORDS]) {
#pragma unroll
    for (int k = 0; k < WORDS; ++k) acc[k] = 0.0;
    for (int t = chain; t < tiles; t += CHAINS) {
        const T* w = p + (size_t)t * stride;
#pragma unroll
        for (int k = 0; k < WORDS; ++k) acc[k] += (double)w[k];
    }
}
template <int CHAINS, typename T>
__device__ __forceinline__ double chain_sum(const T* p, size_t stride, int tiles, int chain) {
    double acc[1];
    chain_sum<CHAINS, 1>(p, stride, tiles, chain, acc);
    return acc[0];
}

// What the kernels that score predicted fields share (gclm_metrics.hip: one calibration per image, gclm_hypotheses.hip: N
// per image): the masked up error in degrees (its formula is in gclm_metrics.hip's header).
constexpr float kDegrees = 57.29577951308232f;
constexpr float kCosEps = 1e-8f;             // F.cosine_similarity's eps

__device__ __forceinline__ float up_error_deg(float px, float py, f32x2 t) {
    const float pn2 = px * px + py * py, tn2 = t.x * t.x + t.y * t.y;
    float dot = px * t.x + py * t.y, crs = px * t.y - py * t.x, sn;
    if (pn2 >= kCosEps * kCosEps && tn2 >= kCosEps * kCosEps) {
        sn = fabsf(crs);
    } else {                                  // a norm below eps (or NaN): the cosine is taken of vectors shorter than 1
        float pn = sqrtf(pn2), tn = sqrtf(tn2);
        pn = pn < kCosEps ? kCosEps : pn;      // clamp_min; a NaN norm stays NaN
        tn = tn < kCosEps ? kCosEps : tn;
        const float ip = 1.f / pn, it = 1.f / tn;
        dot *= ip * it, crs *= ip * it;
        const float n = (pn2 * ip * ip) * (tn2 * it * it), gap = 1.f - n;
        sn = sqrtf((gap > 0.f ? gap : 0.f) + crs * crs);
    }
    const float e = atan2f(sn, dot) * kDegrees;
    return e * (px + py != 0.f ? 1.f : 0.f);  // NaN * 0 = NaN, as torch
}

}  // namespace gclm
