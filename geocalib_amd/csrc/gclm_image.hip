// gclm_image.hip -- gclm_undistort_image, gclm_undistort_image_u8: BaseCamera.undistort_image (reference
// geocalib/camera.py:396-412) in one pass, over float32 or byte images: one kernel template, one launcher template.
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
// s_model is the non-cancelling distort scale of gclm_render.h (not the sweep's float32 form: a resampler is held to float64).
//
// Zero padding as grid_sample's (gclm_render.h: bilinear_taps): a tap outside [0, Win) x [0, Hin) is not read, and a
// non-finite coordinate (NaN or inf camera, or an overflow) contributes nothing: the output pixel is 0.
//
// Layout: one wave walks 64 adjacent output pixels of a row, a block of 4 waves covers 4 rows, grid = (tiles of one image, B).
// No LDS, no scratch, no barrier.  Measured variants (DESIGN.md 3.5, 1920x1080, C = 3, B = 1 / 16 / 64): nontemporal stores
// -3 ... -13 % kernel time, kept; two pixels per lane +23 ... +52 %, the XCD-banded block order +5 ... +11 %, both dropped.
#include "gclm_render.h"

namespace gclm {
namespace {

// One kernel for both element types: T = float reads and writes planar float32 images (INTERLEAVED = false only), T =
// unsigned char byte images, planar or interleaved (gclm_render.h: sample_store_u8).  The coordinate code stands once; the
// tail alone depends on T.  `dwords` (the byte images' dword path, decided by the entry point) comes last, behind every
// argument the float instantiations read: their instruction streams are those of the float-only kernel.
template <int MODEL, typename T, bool INTERLEAVED>
__global__ __launch_bounds__(kBlock) void undistort_image_kernel(const float* __restrict__ cam, int cam_stride,
                                                                 const T* __restrict__ src, int C, int Hin, int Win, int H,
                                                                 int W, int tiles_x, T* __restrict__ dst, int dwords) {
    int x, y;
    if (!tile_pixel(tiles_x, H, W, x, y)) return;
    const int b = blockIdx.y;
    const float* cb = cam + (size_t)b * cam_stride;
    const float fx = cb[2], fy = cb[3], cx = cb[4], cy = cb[5], k1 = cb[6], k2 = cb[7];
    const float ifx = 1.f / fx, ify = 1.f / fy;
    const float sx = (float)(Win - 1) / (float)(W - 1), sy = (float)(Hin - 1) / (float)(H - 1);
    const float dx = (float)x - cx, dy = (float)y - cy;
    const float u = dx * ifx, v = dy * ify;
    float s, sp;
    distort_scale<MODEL>(u * u + v * v, k1, k2, s, sp);
    const Taps a = bilinear_taps((dx * s + cx) * sx, (dy * s + cy) * sy, Hin, Win);
    if constexpr (std::is_same_v<T, float>) {
        const size_t plane_in = (size_t)Hin * Win, plane_out = (size_t)H * W;
        const float* p = src + (size_t)b * C * plane_in;
        // the pixel's offset in its plane fits 32 bits (gclm_undistort_image refuses H W > INT32_MAX); widened before the
        // multiply, the compiler factors W out of image base and row and multiplies a 64-bit vector by it (+8 VALU per lane)
        float* d = dst + (size_t)b * C * plane_out + (y * W + x);
        for (int c = 0; c < C; ++c, p += plane_in, d += plane_out) store_nt(bilinear_sample(p, a, Win), d);
    } else {
        sample_store_u8<INTERLEAVED>(src, dst, a, b, C, Hin, Win, (size_t)H * W, y * W + x, dwords != 0);
    }
}

}  // namespace

template <typename T>
hipError_t launch_undistort_image(int camera_model, const float* cam, int cam_batch, const T* src, int B, int C, int Hin, int Win,
                                  int H, int W, bool interleaved, bool dwords, T* dst, hipStream_t st) {
    return with_camera_model(camera_model, [&](auto m) {
        auto launch = [&](auto il) {
            hipLaunchKernelGGL((undistort_image_kernel<decltype(m)::value, T, decltype(il)::value>), dim3(tile_count(H, W), B),
                               dim3(kBlock), 0, st, cam, cam_batch == 1 ? 0 : 8, src, C, Hin, Win, H, W, tile_columns(W), dst,
                               (int)dwords);
            return hipGetLastError();
        };
        if constexpr (std::is_same_v<T, float>) return launch(std::false_type{});      // (float images are planar)
        else return interleaved ? launch(std::true_type{}) : launch(std::false_type{});
    });
}
template hipError_t launch_undistort_image(int, const float*, int, const float*, int, int, int, int, int, int, bool, bool, float*,
                                           hipStream_t);
template hipError_t launch_undistort_image(int, const float*, int, const unsigned char*, int, int, int, int, int, int, bool, bool,
                                           unsigned char*, hipStream_t);

}  // namespace gclm
