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
// t_model is the undistort scale of gclm_render.h.
//
// Zero padding as grid_sample's (gclm_render.h: bilinear_taps): a tap outside [0, Ws) x [0, Hs) is not read, and a
// non-finite coordinate (a NaN or inf in the camera or the rotation) contributes nothing: the output pixel is 0.
//
// Sources: every image names its own panorama by value in a kernel argument (PanoSrcs, up to kMaxPanoSrcs per launch; a
// pointer may repeat), so n images resampled from one panorama or from n resized copies cost the same single launch.
// Layout: one wave walks 64 adjacent output pixels of a row, a block of 4 waves covers 4 rows, grid = (tiles, images).
// No LDS, no scratch, no barrier.
// Nontemporal stores against plain stores: within the noise here, kept as for undistort.
#include "gclm_render.h"

namespace gclm {
namespace {

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
__global__ __launch_bounds__(kBlock) void render_from_pano_kernel(const float* __restrict__ cam, int cam_stride,
                                                                  const float* __restrict__ rot, const PanoSrcs srcs, int C,
                                                                  int H, int W, int tiles_x, float* __restrict__ dst) {
    int x, y;
    if (!tile_pixel(tiles_x, H, W, x, y)) return;
    const int i = blockIdx.y;
    const float* cb = cam + (size_t)i * cam_stride;
    const float fx = cb[2], fy = cb[3], cx = cb[4], cy = cb[5], k1 = cb[6], k2 = cb[7];
    const float* R = rot + (size_t)i * 9;
    const PanoSrc ps = srcs.s[i];
    const int Hs = ps.h, Ws = ps.w;

    const float u = ((float)x - cx) / fx, v = ((float)y - cy) / fy;
    const float s = undistort_scale<MODEL>(u * u + v * v, k1, k2);
    const float pu = u * s, pv = v * s;
    const float qx = pu * R[0] + pv * R[3] + R[6];
    const float qy = pu * R[1] + pv * R[4] + R[7];
    const float qz = pu * R[2] + pv * R[5] + R[8];
    const float lon = atan2f(qx, qz), lat = atan2f(qy, hypotf(qx, qz));
    const Taps a = bilinear_taps((lon * kInvPi + 1.f) * 0.5f * (float)(Ws - 1), (2.f * lat * kInvPi + 1.f) * 0.5f * (float)(Hs - 1),
                                 Hs, Ws);
    const size_t plane_in = (size_t)Hs * Ws, plane_out = (size_t)H * W;
    const float* p = ps.p;
    float* d = dst + (size_t)i * C * plane_out + (size_t)y * W + x;
    for (int c = 0; c < C; ++c, p += plane_in, d += plane_out) store_nt(bilinear_sample(p, a, Ws), d);
}

}  // namespace

hipError_t launch_render_from_pano(int camera_model, const float* cam, int cam_batch, const float* rot, const float* const* srcs,
                                   const int* src_hw, int n, int C, int H, int W, float* dst, hipStream_t st) {
    return with_camera_model(camera_model, [&](auto m) {
        const size_t per_image = (size_t)C * H * W;
        for (int i0 = 0; i0 < n; i0 += kMaxPanoSrcs) {
            const int k = n - i0 < kMaxPanoSrcs ? n - i0 : kMaxPanoSrcs;
            PanoSrcs tab{};
            for (int j = 0; j < k; ++j) tab.s[j] = PanoSrc{srcs[i0 + j], src_hw[2 * (i0 + j)], src_hw[2 * (i0 + j) + 1]};
            hipLaunchKernelGGL(render_from_pano_kernel<decltype(m)::value>, dim3(tile_count(H, W), k), dim3(kBlock), 0, st,
                               cam + (cam_batch == 1 ? 0 : (size_t)i0 * 8), cam_batch == 1 ? 0 : 8, rot + (size_t)i0 * 9, tab, C,
                               H, W, tile_columns(W), dst + (size_t)i0 * per_image);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    });
}

}  // namespace gclm
