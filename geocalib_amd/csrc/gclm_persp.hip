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
// persp_up / persp_lat (the two formulas above) and s, s' (distort scale and ds/dr2), t (undistort scale) per model are
// gclm_render.h's: the reference's definitions in forms that do not cancel in float32, held to float64
// (tests/perspective_gate.py).  gclm_metrics.hip scores fields against the same text.
//
// NaN: a NaN or inf in the camera or gravity gives NaN wherever the torch composition gives NaN.  Both guards (the norm's
// 1e-12 floor and the clamp) are comparisons that keep a NaN operand, not fminf / fmaxf, which would drop it.
//
// Layout: up (B, H, W, 2) interleaved, lat (B, H, W, 1); either may be NULL.  One wave walks 128 adjacent pixels of a row
// (64 where W is odd), a block of 4 waves covers 4 rows, grid = (tiles of one image, B).  64-bit offsets.  No LDS, no scratch, no barrier.
// Measured variants (DESIGN.md 3.7, 640x480, B = 1024, against one pixel per lane with plain stores): two pixels per lane
// -16 % (pinhole) / -8 % (simple_divisional) kernel time, with nontemporal stores on top -22 % / -10 %: both kept.  Two
// pixels per lane (dwordx4 / dwordx2 stores) run where W is even and the outputs are 16 / 8 byte aligned, one otherwise.
#include "gclm_render.h"

namespace gclm {
namespace {

template <int MODEL, int PX>
__global__ __launch_bounds__(kBlock) void perspective_field_kernel(const float* __restrict__ cam, const float* __restrict__ grav,
                                                                   int H, int W, int tiles_x, int normalize,
                                                                   float* __restrict__ up, float* __restrict__ lat) {
    int x, y;
    if (!tile_pixel<PX>(tiles_x, H, W, x, y)) return;
    const int b = blockIdx.y;
    const PerspRow r = persp_row(cam + (size_t)b * 8, grav + (size_t)b * 3, y);
    const size_t o = ((size_t)b * H + y) * W + x;
    const bool nrm = normalize != 0;
    if constexpr (PX == 1) {
        const float u = ((float)x - r.cx) * r.ifx, r2 = u * u + r.v2;
        if (up) store_nt(persp_up<MODEL>(r, u, r2, nrm), reinterpret_cast<f32x2*>(up + 2 * o));
        if (lat) store_nt(persp_lat<MODEL>(r, u, r2), lat + o);
    } else {
        // PX = 2 runs only for even W with 16-byte aligned up and 8-byte aligned lat: x is even, so x + 1 < W and o is even
        const float u0 = ((float)x - r.cx) * r.ifx, u1 = ((float)(x + 1) - r.cx) * r.ifx;
        const float r20 = u0 * u0 + r.v2, r21 = u1 * u1 + r.v2;
        if (up) {
            const f32x2 e = persp_up<MODEL>(r, u0, r20, nrm), f = persp_up<MODEL>(r, u1, r21, nrm);
            store_nt(f32x4{e.x, e.y, f.x, f.y}, reinterpret_cast<f32x4*>(up + 2 * o));
        }
        if (lat) store_nt(f32x2{persp_lat<MODEL>(r, u0, r20), persp_lat<MODEL>(r, u1, r21)}, reinterpret_cast<f32x2*>(lat + o));
    }
}

}  // namespace

hipError_t launch_perspective_fields(int camera_model, const float* cam, const float* grav, int B, int H, int W, int normalize,
                                     float* up, float* lat, hipStream_t st) {
    // two pixels per lane need x + 1 < W for every even x and vector stores that are aligned
    const bool two = W % 2 == 0 && reinterpret_cast<uintptr_t>(up) % 16 == 0 && reinterpret_cast<uintptr_t>(lat) % 8 == 0;
    return with_camera_model(camera_model, [&](auto m) {
        constexpr int M = decltype(m)::value;
        const auto kernel = two ? perspective_field_kernel<M, 2> : perspective_field_kernel<M, 1>;
        const int px = two ? 2 : 1;
        hipLaunchKernelGGL(kernel, dim3(tile_count(H, W, px), B), dim3(kBlock), 0, st, cam, grav, H, W, tile_columns(W, px),
                           normalize, up, lat);
        return hipGetLastError();
    });
}

}  // namespace gclm
