// gclm_reproject.hip -- gclm_reproject_image, gclm_reproject_image_u8: BaseCamera.reproject_image / upright_image in one pass,
// over float32 or byte images (one kernel template, one launcher template): an image as another camera, turned by a rotation,
// sees it.  It joins the halves its siblings use: the target pixel's ray as
// gclm_render_from_pano takes it (the undistort form), the source pixel of that ray as gclm_undistort_image takes it (the
// distort form).
//
// On the torch path this is about twenty elementwise launches (pixel grid, image2world, the rotation, project, distort and
// its derivative, denormalize, the masks) and F.grid_sample(bilinear, zeros, align_corners=True).  Here each lane computes
// its output pixel's source coordinate in registers, once for all channels, and loops over the channels with the four
// taps' offsets and weights held.  Per output pixel (x, y), integer pixel centres, no half-pixel offset, float32:
//   u = (x - cx_t) / fx_t,  v = (y - cy_t) / fy_t,  r2 = u^2 + v^2
//   t = undistort scale of the TARGET model at r2              (gclm_render.h)
//   b = (u t, v t, 1)                                          (not normalised)
//   q = b M          row vector times M (n, 3, 3) row-major, the convention of gclm_render_from_pano; M NULL: q = b
//   visible = q_z > 1e-3                                       (BaseCamera.eps, the reference's project())
//   p = (q_x, q_y) / q_z,  r2s = |p|^2
//   (s, s') = distort scale of the SOURCE model at r2s and ds/dr2, the non-cancelling forms of gclm_render.h
//   inside_model = s + 2 r2s s' > 0
//   ix = (p_x s fx_s + cx_s) (Win - 1) / (Ws - 1),   iy = (p_y s fy_s + cy_s) (Hin - 1) / (Hs - 1)
// inside_model says that r s(r^2) still increases: beyond that radius a polynomial model folds far rays back into the
// image.  Pinhole is always inside.  Ws x Hs is the nominal size of the source camera (integers from the host), Win x Hin
// the size the image is stored at, as for gclm_undistort_image.
//
// The output is the bilinear sample with zero padding (gclm_render.h: bilinear_taps), exactly 0 where visible or
// inside_model fails and exactly 0 where a coordinate is not finite.  A non-finite camera or rotation entry zeroes its whole
// image: a NaN fails every comparison; an infinite target focal (whose reciprocal would be a clean 0) is turned into a NaN,
// and an infinite q_z (which would divide to a clean 0) counts as invisible.  valid (optional, uint8) is 1 iff
// visible && inside_model && 0 <= ix <= Win - 1 && 0 <= iy <= Hin - 1.
//
// Layout: one wave walks 64 adjacent output pixels of a row, a block of 4 waves covers 4 rows, grid = (tiles of one image, B).
// No LDS, no scratch, no barrier.  The camera rows and the rotation depend on blockIdx alone: scalar loads.  Nontemporal
// stores as in the two siblings.  Measured: DESIGN.md 3.12.
#include <cfloat>

#include "gclm_render.h"

namespace gclm {
namespace {

constexpr float kVisibleEps = 1e-3f;       // BaseCamera.eps

// One kernel for both element types: T = float reads and writes planar float32 images (INTERLEAVED = false only), T =
// unsigned char byte images, planar or interleaved (gclm_render.h: sample_store_u8).  The coordinate code, the visibility and
// fold-back rules and the mask stand once; the tail alone depends on T.  `dwords` (the byte images' dword path, decided by
// the entry point) comes last, behind every argument the float instantiations read: their instruction streams are those of
// the float-only kernel.
template <int SRC_MODEL, int DST_MODEL, bool HAS_ROT, typename T, bool INTERLEAVED>
__global__ __launch_bounds__(kBlock) void reproject_kernel(const float* __restrict__ src_cam, const float* __restrict__ dst_cam,
                                                           int cam_stride, const float* __restrict__ rot, int rot_stride,
                                                           const T* __restrict__ src, int C, int Hin, int Win, int Hs, int Ws,
                                                           int H, int W, int tiles_x, T* __restrict__ dst,
                                                           unsigned char* __restrict__ valid, int dwords) {
    int x, y;
    if (!tile_pixel(tiles_x, H, W, x, y)) return;
    const int b = blockIdx.y;
    const float* ct = dst_cam + (size_t)b * cam_stride;
    const float* cs = src_cam + (size_t)b * cam_stride;
    const float fxt = ct[2], fyt = ct[3], cxt = ct[4], cyt = ct[5];
    const float fxs = cs[2], fys = cs[3], cxs = cs[4], cys = cs[5];
    // 1 / inf = 0 would look straight ahead from every pixel: 0 * inf = NaN keeps an infinite focal non-finite
    const float ifx = 1.f / fxt + 0.f * fxt, ify = 1.f / fyt + 0.f * fyt;
    const float sx = (float)(Win - 1) / (float)(Ws - 1), sy = (float)(Hin - 1) / (float)(Hs - 1);

    const float u = ((float)x - cxt) * ifx, v = ((float)y - cyt) * ify;
    const float t = undistort_scale<DST_MODEL>(u * u + v * v, ct[6], ct[7]);
    const float bu = u * t, bv = v * t;
    float qx = bu, qy = bv, qz = 1.f;
    if constexpr (HAS_ROT) {
        const float* M = rot + (size_t)b * rot_stride;
        qx = bu * M[0] + bv * M[3] + M[6];
        qy = bu * M[1] + bv * M[4] + M[7];
        qz = bu * M[2] + bv * M[5] + M[8];
    }
    bool ok = qz > kVisibleEps && qz <= FLT_MAX;
    const float iz = 1.f / qz, px = qx * iz, py = qy * iz, r2s = px * px + py * py;
    float s, sp;
    distort_scale<SRC_MODEL>(r2s, cs[6], cs[7], s, sp);
    if constexpr (SRC_MODEL != GCLM_PINHOLE) ok = ok && s + 2.f * r2s * sp > 0.f;
    const float ix = (px * s * fxs + cxs) * sx, iy = (py * s * fys + cys) * sy;
    // an invisible or folded pixel samples where no tap lies inside the source
    const Taps a = bilinear_taps(ok ? ix : -2.f, ok ? iy : -2.f, Hin, Win);

    const size_t plane_out = (size_t)H * W;
    const int o = y * W + x;                  // fits 32 bits: gclm_reproject_image refuses H W > INT32_MAX
    if (valid) {
        const bool in = ok && ix >= 0.f && ix <= (float)(Win - 1) && iy >= 0.f && iy <= (float)(Hin - 1);
        store_nt((unsigned char)in, valid + (size_t)b * plane_out + o);
    }
    if constexpr (std::is_same_v<T, float>) {
        const size_t plane_in = (size_t)Hin * Win;
        const float* p = src + (size_t)b * C * plane_in;
        float* d = dst + (size_t)b * C * plane_out + o;
        for (int c = 0; c < C; ++c, p += plane_in, d += plane_out) store_nt(bilinear_sample(p, a, Win), d);
    } else {
        sample_store_u8<INTERLEAVED>(src, dst, a, b, C, Hin, Win, plane_out, o, dwords != 0);
    }
}

}  // namespace

template <typename T>
hipError_t launch_reproject_image(int src_model, const float* src_cam, int dst_model, const float* dst_cam, int cam_batch,
                                  const float* rot, int rot_batch, const T* src, int B, int C, int Hin, int Win, int Hs, int Ws,
                                  int H, int W, bool interleaved, bool dwords, T* dst, unsigned char* valid, hipStream_t st) {
    return with_camera_model(src_model, [&](auto ms) {
        return with_camera_model(dst_model, [&](auto mt) {
            auto launch = [&](auto has_rot, auto il) {
                hipLaunchKernelGGL((reproject_kernel<decltype(ms)::value, decltype(mt)::value, decltype(has_rot)::value, T,
                                                     decltype(il)::value>),
                                   dim3(tile_count(H, W), B), dim3(kBlock), 0, st, src_cam, dst_cam, cam_batch == 1 ? 0 : 8, rot,
                                   rot_batch == 1 ? 0 : 9, src, C, Hin, Win, Hs, Ws, H, W, tile_columns(W), dst, valid, (int)dwords);
                return hipGetLastError();
            };
            auto layout = [&](auto has_rot) {
                if constexpr (std::is_same_v<T, float>) return launch(has_rot, std::false_type{});     // (float images are planar)
                else return interleaved ? launch(has_rot, std::true_type{}) : launch(has_rot, std::false_type{});
            };
            return rot ? layout(std::true_type{}) : layout(std::false_type{});
        });
    });
}
template hipError_t launch_reproject_image(int, const float*, int, const float*, int, const float*, int, const float*, int, int, int,
                                           int, int, int, int, int, bool, bool, float*, unsigned char*, hipStream_t);
template hipError_t launch_reproject_image(int, const float*, int, const float*, int, const float*, int, const unsigned char*, int,
                                           int, int, int, int, int, int, int, bool, bool, unsigned char*, unsigned char*, hipStream_t);

}  // namespace gclm
