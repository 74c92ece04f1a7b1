// gclm_pano.hip -- gclm_render_from_pano: BaseCamera.get_img_from_pano (reference geocalib/camera.py:414-514) in one pass.
//
// The reference renders each perspective image from an equirectangular panorama with a chain of about fifteen torch ops
// (pixel grid, image2world, F.normalize, bearings @ gravity.R @ R_yaw, two atan2, a norm, the pano_shape affine and
// F.grid_sample(bilinear, zeros, align_corners=True)).  Here each lane computes its output pixel's panorama coordinate in
// registers, once for all channels, and loops over the channels with the four taps' offsets and weights held:
//   u = (x - cx) / fx,  v = (y - cy) / fy,  r2 = u^2 + v^2,  t = t_model(r2)           (image2world: the undistort form)
//   q = (u t, v t, 1) R_i                                                              (row vector times R_i)
//   lon = atan2(q_x, q_z),  lat = atan2(q_y, hypot(q_x, q_z))
//   ix = (lon / pi + 1) / 2 (Ws - 1),   iy = (2 lat / pi + 1) / 2 (Hs - 1)
// Integer pixel centres, no half-pixel offset.  The reference normalises the bearing before the rotation; both angles are
// invariant to a positive scale of q, so the normalisation is skipped (one sqrt and three divisions fewer per pixel, and
// no extra rounding).  R_i = gravity.R[i] @ rad2rotmat(0, 0, yaw_i) arrives from the host as a (n, 3, 3) float32 tensor:
// the kernel knows nothing of gravity or yaw.  The pano_shape bookkeeping of the reference cancels exactly, so the sample
// point depends on the (resized) panorama's own Hs x Ws only.  Longitude does not wrap at +-pi (the reference's
// grid_sample pads with zeros there too).
//
// t_model: pinhole 1; simple_radial 1 - k1 r2; radial 1 - k1 r2 + (3 k1^2 - k2) r2^2; simple_divisional 1 / (1 + k1 r2),
// with a zero denominator replaced by 1e6 (the reference's masked_fill).
//
// Zero padding as grid_sample's: each tap contributes only if it lies in [0, Ws) x [0, Hs), and is not read otherwise.  A
// non-finite coordinate (a NaN or inf in the camera or the rotation) contributes nothing: the output pixel is 0.
//
// Sources: every image names its own panorama by value in a kernel argument (PanoSrcs, up to kMaxPanoSrcs per launch; a
// pointer may repeat), so n images resampled from one panorama or from n resized copies cost the same single launch.
// Layout: one wave walks 64 adjacent output pixels of a row, a block of 4 waves covers 4 rows, grid = (tiles, images).
// No LDS, no scratch, no barrier.
#include "gclm_internal.h"

#ifndef GCLM_PANO_NT
#define GCLM_PANO_NT 1          // 1: nontemporal stores to the destination (0: plain stores), DESIGN.md 3.6
#endif

namespace gclm {
namespace {

constexpr int kRows = 4;                  // rows per block: one per wave
constexpr int kMaxPanoSrcs = 192;         // panoramas per launch: 192 x 16 B = 3 KB of the 4 KB kernel-argument space

struct PanoSrc {
    const float* p;
    int h, w;
};
struct PanoSrcs {
    PanoSrc s[kMaxPanoSrcs];
};
static_assert(sizeof(PanoSrcs) + 64 <= 4096, "the panorama table must fit the kernel-argument space with the other args");

constexpr float kInvPi = 0.318309886183790671538f;

template <int MODEL>
__device__ __forceinline__ float pano_undistort_scale(float r2, float k1, float k2) {
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

template <bool NT>
__device__ __forceinline__ void pano_store(float v, float* p) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <int MODEL, bool NT>
__global__ __launch_bounds__(kBlock) void render_from_pano_kernel(const float* __restrict__ cam, int cam_stride,
                                                                  const float* __restrict__ rot, const PanoSrcs srcs, int C,
                                                                  int H, int W, int tiles_x, int tiles, float* __restrict__ dst) {
    const int t = blockIdx.x;
    if (t >= tiles) return;
    const int i = blockIdx.y;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y = ty * kRows + (threadIdx.x >> 6);
    const int x = tx * 64 + (threadIdx.x & 63);
    if (y >= H || x >= W) return;
    const float* cb = cam + (size_t)i * cam_stride;
    const float fx = cb[2], fy = cb[3], cx = cb[4], cy = cb[5], k1 = cb[6], k2 = cb[7];
    const float* R = rot + (size_t)i * 9;
    const PanoSrc ps = srcs.s[i];
    const int Hs = ps.h, Ws = ps.w;

    const float u = ((float)x - cx) / fx, v = ((float)y - cy) / fy;
    const float s = pano_undistort_scale<MODEL>(u * u + v * v, k1, k2);
    const float pu = u * s, pv = v * s;
    const float qx = pu * R[0] + pv * R[3] + R[6];
    const float qy = pu * R[1] + pv * R[4] + R[7];
    const float qz = pu * R[2] + pv * R[5] + R[8];
    const float lon = atan2f(qx, qz), lat = atan2f(qy, hypotf(qx, qz));
    float ix = (lon * kInvPi + 1.f) * 0.5f * (float)(Ws - 1);
    float iy = (2.f * lat * kInvPi + 1.f) * 0.5f * (float)(Hs - 1);
    // NaN -> -2, +-inf -> just outside the panorama: every tap then lies outside and the pixel is 0
    ix = ix == ix ? fminf(fmaxf(ix, -2.f), (float)Ws + 1.f) : -2.f;
    iy = iy == iy ? fminf(fmaxf(iy, -2.f), (float)Hs + 1.f) : -2.f;
    const float x0 = floorf(ix), y0 = floorf(iy);
    const int xi = (int)x0, yi = (int)y0;
    const float ax = ix - x0, ay = iy - y0, bx = 1.f - ax, by = 1.f - ay;
    const bool mx0 = (unsigned)xi < (unsigned)Ws, mx1 = (unsigned)(xi + 1) < (unsigned)Ws;
    const bool my0 = (unsigned)yi < (unsigned)Hs, my1 = (unsigned)(yi + 1) < (unsigned)Hs;
    const bool m00 = mx0 && my0, m01 = mx1 && my0, m10 = mx0 && my1, m11 = mx1 && my1;
    const float w00 = bx * by, w01 = ax * by, w10 = bx * ay, w11 = ax * ay;        // grid_sample's nw, ne, sw, se
    const int64_t o = (int64_t)yi * Ws + xi;
    const size_t plane_in = (size_t)Hs * Ws, plane_out = (size_t)H * W;
    const float* p = ps.p;
    float* d = dst + (size_t)i * C * plane_out + (size_t)y * W + x;
    for (int c = 0; c < C; ++c, p += plane_in, d += plane_out) {
        const float v00 = m00 ? p[o] : 0.f, v01 = m01 ? p[o + 1] : 0.f;
        const float v10 = m10 ? p[o + Ws] : 0.f, v11 = m11 ? p[o + Ws + 1] : 0.f;
        pano_store<NT>(v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11, d);
    }
}

template <int MODEL>
hipError_t launch_pano_model(const float* cam, int cam_batch, const float* rot, const float* const* srcs, const int* src_hw,
                             int n, int C, int H, int W, float* dst, hipStream_t st) {
    const int tiles_x = (W + 63) / 64, tiles = tiles_x * ((H + kRows - 1) / kRows);
    const size_t per_image = (size_t)C * H * W;
    for (int i0 = 0; i0 < n; i0 += kMaxPanoSrcs) {
        const int m = n - i0 < kMaxPanoSrcs ? n - i0 : kMaxPanoSrcs;
        PanoSrcs tab{};
        for (int j = 0; j < m; ++j) tab.s[j] = PanoSrc{srcs[i0 + j], src_hw[2 * (i0 + j)], src_hw[2 * (i0 + j) + 1]};
        hipLaunchKernelGGL((render_from_pano_kernel<MODEL, GCLM_PANO_NT != 0>), dim3(tiles, m), dim3(kBlock), 0, st,
                           cam + (cam_batch == 1 ? 0 : (size_t)i0 * 8), cam_batch == 1 ? 0 : 8, rot + (size_t)i0 * 9, tab, C,
                           H, W, tiles_x, tiles, dst + (size_t)i0 * per_image);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

}  // namespace
}  // namespace gclm

extern "C" int gclm_render_from_pano(int camera_model, const float* d_cam, int cam_batch, const float* d_rot,
                                     const float* const* srcs, const int* src_hw, int n, int C, int H, int W, float* d_dst,
                                     void* stream) {
    using namespace gclm;
    // every check runs before the first HIP call
    if (!d_cam || !d_rot || !srcs || !src_hw || !d_dst || n < 1 || n > 65535 || C < 1 || H < 2 || W < 2) return -3;
    if ((cam_batch != 1 && cam_batch != n) || camera_model < GCLM_PINHOLE || camera_model > GCLM_SIMPLE_DIVISIONAL) return -3;
    if ((int64_t)H * W > INT32_MAX) return -3;
    const size_t out_bytes = (size_t)n * C * H * W * sizeof(float);
    if (overlaps(d_dst, out_bytes, d_cam, (size_t)cam_batch * 8 * sizeof(float)) ||
        overlaps(d_dst, out_bytes, d_rot, (size_t)n * 9 * sizeof(float)))
        return -3;
    for (int i = 0; i < n; ++i) {
        const int Hs = src_hw[2 * i], Ws = src_hw[2 * i + 1];
        if (!srcs[i] || Hs < 2 || Ws < 2) return -3;
        if (overlaps(d_dst, out_bytes, srcs[i], (size_t)C * Hs * Ws * sizeof(float))) return -3;
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e;
    switch (camera_model) {
        case GCLM_PINHOLE: e = launch_pano_model<GCLM_PINHOLE>(d_cam, cam_batch, d_rot, srcs, src_hw, n, C, H, W, d_dst, st); break;
        case GCLM_SIMPLE_RADIAL:
            e = launch_pano_model<GCLM_SIMPLE_RADIAL>(d_cam, cam_batch, d_rot, srcs, src_hw, n, C, H, W, d_dst, st);
            break;
        case GCLM_RADIAL: e = launch_pano_model<GCLM_RADIAL>(d_cam, cam_batch, d_rot, srcs, src_hw, n, C, H, W, d_dst, st); break;
        default:
            e = launch_pano_model<GCLM_SIMPLE_DIVISIONAL>(d_cam, cam_batch, d_rot, srcs, src_hw, n, C, H, W, d_dst, st);
            break;
    }
    return e == hipSuccess ? 0 : -10;
}
