// gclm_overlay.hip -- gclm_draw_fields, gclm_draw_fields_u8: the perspective fields of a calibration drawn over a batch of
// images (viz.draw_perspective_fields), in one pass that reads a frame once and writes it once.  The reference's demo does this
// on the host (interactive_demo.py: plot_confidence, plot_latitude, draw_horizon_line, plot_vector_field): both fields
// rendered, a matplotlib colormap, cv2.addWeighted, cv2.findContours once per level, cv2.line, cv2.arrowedLine.  Every layer
// of that picture is a function of one output pixel, its calibration and at most one confidence value, so a lane here
// evaluates its pixel's latitude, the latitude's slope in degrees per pixel (gclm_render.h: persp_lat, persp_lat_slope) and
// the up vectors of the four arrow anchors of its cell (persp_up) in registers and composites the layers in order:
//   heat -> tint -> contours -> horizon -> arrows,   out = out (1 - a) + colour a        (definition: include/gclm.h)
// A line's coverage a is clamp(halfwidth + 0.5 - d, 0, 1) with d the distance in pixels to the isoline (|lat - level| / slope)
// or to the nearest of an arrow's three segments.  This is the demo's picture antialiased, not cv2's rasteriser.
//
// NaN: every guard is a comparison that fails on NaN, so a non-finite latitude, slope, confidence or anchor skips its layer
// and a NaN calibration copies the image.  With no layer on the pixel is stored as loaded.
//
// Layout: the tile geometry of gclm_render.h (a wave walks 64 adjacent pixels of a row, a block 4 rows, grid = (tiles, B)), one
// pixel per lane.  No LDS, no barrier, no scratch: a palette lookup is six byte loads of a 768-byte table that stays in the
// caches (staging both palettes per block into LDS as packed dwords was measured and took 3 - 17 % longer: DESIGN.md 3.14).  The
// layer set is a kernel argument and branches wave-uniformly: 4 models x {float planar, byte planar, byte interleaved} = 12
// instantiations.  The style arrives by value.
// Byte stores as sample_store_u8 does them; interleaved C = 4 on dword boundaries loads and stores one dword per pixel.
// Measured: DESIGN.md 3.14.
#include <cfloat>

#include "gclm_render.h"

namespace gclm {
namespace {

// pal(L, tau) of include/gclm.h on a (256, 3) byte palette; tau is finite and in [0, 1] up to rounding.
__device__ __forceinline__ void palette_colour(const unsigned char* __restrict__ L, float tau, float (&c)[3]) {
    const float p = 255.f * tau;
    int i = (int)p;
    i = i < 0 ? 0 : (i > 254 ? 254 : i);
    const float f = p - (float)i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = (float)L[3 * i + k], b = (float)L[3 * i + 3 + k];
        c[k] = a + (b - a) * f;
    }
}

__device__ __forceinline__ void blend(float (&o)[3], const float (&c)[3], float a, float unit) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = o[k] * (1.f - a) + c[k] * unit * a;
}

// coverage of a line of half-width hw at distance d: NaN gives 0
__device__ __forceinline__ float coverage(float hw, float d) {
    const float a = hw + 0.5f - d;
    return a > 0.f ? (a < 1.f ? a : 1.f) : 0.f;
}

// distance from w = P - A to the segment A + s D, s in [0, 1]
__device__ __forceinline__ float segment_distance(float wx, float wy, float dx, float dy) {
    const float len2 = dx * dx + dy * dy;
    float s = len2 > 0.f ? (wx * dx + wy * dy) / len2 : 0.f;
    s = s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
    const float ex = wx - s * dx, ey = wy - s * dy;
    return sqrtf(ex * ex + ey * ey);
}

// The arrows' coverage of pixel (x, y): the largest over the four anchors of its cell.  `r` holds the image's terms; the
// anchor's row terms are rebuilt here.
template <int MODEL>
__device__ __forceinline__ float arrow_coverage(const PerspRow& r, float cy, float ify, const gclm_overlay_style& st, int x, int y,
                                                int H, int W) {
    const int S = st.arrow_step;
    const int i0 = x >= st.arrow_x0 ? (x - st.arrow_x0) / S : -1, j0 = y >= st.arrow_y0 ? (y - st.arrow_y0) / S : -1;
    const float L = st.arrow_length, reach = L + st.arrow_halfwidth + 0.5f, tipL = st.arrow_tip * L * 0.70710678f;
    float best = 0.f;
#pragma unroll
    for (int dj = 0; dj < 2; ++dj) {
#pragma unroll
        for (int di = 0; di < 2; ++di) {
            const int i = i0 + di, j = j0 + dj;
            // (64-bit: x0 + i S may pass 2^31 for a far anchor that is then outside the image)
            const int64_t ax = (int64_t)st.arrow_x0 + (int64_t)i * S, ay = (int64_t)st.arrow_y0 + (int64_t)j * S;
            if (i < 0 || j < 0 || ax >= W || ay >= H) continue;
            const float wx = (float)(x - (int)ax), wy = (float)(y - (int)ay);
            if (!(fabsf(wx) < reach && fabsf(wy) < reach)) continue;       // beyond the arrow's reach: coverage 0
            PerspRow ra = r;
            persp_set_row(ra, ((float)(int)ay - cy) * ify);
            const float u = ((float)(int)ax - r.cx) * r.ifx;
            const f32x2 q = persp_up<MODEL>(ra, u, u * u + ra.v2, false);
            const float n = sqrtf(q.x * q.x + q.y * q.y);
            if (!(n >= 1e-6f && n <= FLT_MAX)) continue;
            const float ex = q.x / n, ey = q.y / n;
            // every segment lies in the box [0, L] x [-tipL, tipL] along and across e: beyond it by the line's reach the coverage is 0
            const float along = wx * ex + wy * ey, across = fabsf(wx * ey - wy * ex), rim = st.arrow_halfwidth + 0.5f;
            if (!(along > -rim && along < L + rim && across < tipL + rim)) continue;
            float d = segment_distance(wx, wy, L * ex, L * ey);
            const float tx = wx - L * ex, ty = wy - L * ey;                // from the tip P1
            d = fminf(d, segment_distance(tx, ty, tipL * (-ex - ey), tipL * (-ey + ex)));      // -e + e_perp, e_perp = (-e_y, e_x)
            d = fminf(d, segment_distance(tx, ty, tipL * (-ex + ey), tipL * (-ey - ex)));      // -e - e_perp
            best = fmaxf(best, coverage(st.arrow_halfwidth, d));
        }
    }
    return best;
}

template <int MODEL, typename T, bool INTERLEAVED>
__global__ __launch_bounds__(kBlock) void overlay_kernel(const float* __restrict__ cam, const float* __restrict__ grav, int cam_stride,
                                                         int grav_stride, const T* __restrict__ src, int C, int H, int W, int tiles_x,
                                                         const float* __restrict__ conf, const unsigned char* __restrict__ palette,
                                                         const unsigned char* __restrict__ heat_palette, gclm_overlay_style st,
                                                         T* __restrict__ dst, int dwords) {
    const unsigned layers = st.layers;
    int x, y;
    if (!tile_pixel(tiles_x, H, W, x, y)) return;
    const int b = blockIdx.y;
    const size_t plane = (size_t)H * W;
    const int o = y * W + x;                  // fits 32 bits: the entry refuses H W > INT32_MAX
    constexpr bool kBytes = !std::is_same_v<T, float>;
    constexpr float unit = kBytes ? 1.f : 1.f / 255.f;       // a colour byte in the image's units

    // the pixel as it lies
    float out[3];
    unsigned word = 0;
    const T* s0;
    T* d0;
    size_t cstep;
    if constexpr (INTERLEAVED) {
        s0 = src + ((size_t)b * plane + o) * C, d0 = dst + ((size_t)b * plane + o) * C, cstep = 1;
    } else {
        s0 = src + (size_t)b * C * plane + o, d0 = dst + (size_t)b * C * plane + o, cstep = plane;
    }
    if (INTERLEAVED && dwords) {
        if constexpr (kBytes) {
            word = *reinterpret_cast<const unsigned*>(s0);
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = (float)((word >> (8 * k)) & 255u);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = (float)s0[k * cstep];
    }

    if (layers) {
        const float* cb = cam + (size_t)b * cam_stride;
        const float* gb = grav + (size_t)b * grav_stride;
        const float ify = 1.f / cb[3], cy = cb[5];     // (persp_row's own: kept for the slope and the anchors' rows)
        const PerspRow r = persp_row(cb, gb, y);
        float col[3];

        if (layers & GCLM_OVERLAY_HEAT) {
            const float c = conf[(size_t)b * plane + o];
            if (fabsf(c) <= FLT_MAX) {
                float l = log10f(c > 1e-6f ? c : 1e-6f);
                l = l < st.heat_lo ? st.heat_lo : (l > st.heat_hi ? st.heat_hi : l);
                palette_colour(heat_palette, (l - st.heat_lo) / (st.heat_hi - st.heat_lo), col);
                blend(out, col, st.heat_alpha, unit);
            }
        }
        if (layers & (GCLM_OVERLAY_TINT | GCLM_OVERLAY_CONTOURS | GCLM_OVERLAY_HORIZON)) {
            const float u = ((float)x - r.cx) * r.ifx, r2 = u * u + r.v2;
            const float lat = persp_lat<MODEL>(r, u, r2) * kDegrees;
            if (fabsf(lat) <= FLT_MAX) {
                if (layers & GCLM_OVERLAY_TINT) {
                    palette_colour(palette, (lat + 90.f) * (1.f / 180.f), col);
                    blend(out, col, st.tint_alpha, unit);
                }
                if (layers & (GCLM_OVERLAY_CONTOURS | GCLM_OVERLAY_HORIZON)) {
                    const float g = persp_lat_slope<MODEL>(r, u, r2, ify);
                    if (fabsf(g) <= FLT_MAX) {
                        const float ig = 1.f / (g > 1e-4f ? g : 1e-4f);
                        if (layers & GCLM_OVERLAY_CONTOURS) {
                            const float last = (float)(st.levels - 1), step = 180.f / last;
                            const float k = __builtin_rintf((lat + 90.f) / step);
                            // level k = -90 + k step as (2 k - last) 90 / last: one rounding, relative to the level, exact at 0
                            const float level = (2.f * k - last) * 90.f / last;
                            const float a = coverage(st.line_halfwidth, fabsf(lat - level) * ig);
                            if (a > 0.f) {
                                palette_colour(palette, k / last, col);
                                blend(out, col, a, unit);
                            }
                        }
                        if (layers & GCLM_OVERLAY_HORIZON) {
                            const float a = coverage(st.line_halfwidth, fabsf(lat) * ig);
#pragma unroll
                            for (int k = 0; k < 3; ++k) col[k] = (float)st.horizon_rgba[k];
                            if (a > 0.f) blend(out, col, a, unit);
                        }
                    }
                }
            }
        }
        if (layers & GCLM_OVERLAY_ARROWS) {
            const float a = arrow_coverage<MODEL>(r, cy, ify, st, x, y, H, W);
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] = (float)st.arrow_rgba[k];
            if (a > 0.f) blend(out, col, a, unit);
        }
    }

    if constexpr (kBytes) {
        if (INTERLEAVED && dwords) {
            const unsigned w = (unsigned)to_u8(out[0]) | (unsigned)to_u8(out[1]) << 8 | (unsigned)to_u8(out[2]) << 16 | (word & 0xff000000u);
            store_nt(w, reinterpret_cast<unsigned*>(d0));
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) store_nt(to_u8(out[k]), d0 + k * cstep);
            if (C == 4) store_nt(s0[3 * cstep], d0 + 3 * cstep);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) store_nt(out[k], d0 + k * cstep);
        if (C == 4) store_nt(s0[3 * cstep], d0 + 3 * cstep);
    }
}

}  // namespace

template <typename T>
hipError_t launch_draw_fields(int camera_model, const float* cam, const float* grav, int cal_batch, const T* src, int B, int C, int H,
                              int W, bool interleaved, bool dwords, const float* conf, const unsigned char* palette,
                              const unsigned char* heat_palette, const gclm_overlay_style& style, T* dst, hipStream_t st) {
    return with_camera_model(camera_model, [&](auto m) {
        auto launch = [&](auto il) {
            hipLaunchKernelGGL((overlay_kernel<decltype(m)::value, T, decltype(il)::value>), dim3(tile_count(H, W), B), dim3(kBlock), 0,
                               st, cam, grav, cal_batch == 1 ? 0 : 8, cal_batch == 1 ? 0 : 3, src, C, H, W, tile_columns(W), conf,
                               palette, heat_palette, style, dst, (int)dwords);
            return hipGetLastError();
        };
        if constexpr (std::is_same_v<T, float>) return launch(std::false_type{});     // (float images are planar)
        else return interleaved ? launch(std::true_type{}) : launch(std::false_type{});
    });
}
template hipError_t launch_draw_fields(int, const float*, const float*, int, const float*, int, int, int, int, bool, bool, const float*,
                                       const unsigned char*, const unsigned char*, const gclm_overlay_style&, float*, hipStream_t);
template hipError_t launch_draw_fields(int, const float*, const float*, int, const unsigned char*, int, int, int, int, bool, bool,
                                       const float*, const unsigned char*, const unsigned char*, const gclm_overlay_style&,
                                       unsigned char*, hipStream_t);

}  // namespace gclm
